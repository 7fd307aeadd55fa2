// rekey_host_check.cpp — the host side of K-rekey (pdl_rekey.h: rk_exact, rk_plan — digit map, table, the two reciprocals) run
// through every key it is easy to get wrong, as a program of its own so that it can be built with the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/rekey_host_check.cpp -o rekey_host_check && ./rekey_host_check
//
// No device is touched: the kernel's arithmetic (rk_items) is repeated here in 128-bit host integers and checked against plain
// division, for alphabets of 1 .. 256 letters at the largest exact k and a few below, growing and shrinking.
#include "../pandelos_amd/csrc/pdl_rekey.h"

#include <cinttypes>
#include <cstring>
#include <random>

static uint64_t mulhi(uint64_t a, uint64_t b) { return (uint64_t) (((unsigned __int128) a * b) >> 64); }

// RankParams of the alphabet `present` as rank_init makes the fields the plan reads (dense digits in byte order, B, k)
static RankParams params_of(const uint8_t present[256], uint32_t k) {
    RankParams rp{};
    uint32_t r = 0;
    for (int b = 0; b < 256; b++) if (present[b]) rp.rank_values[b] = (uint8_t) r++;
    rp.base = r; rp.k = k;
    return rp;
}

// rk_items for one key on the host; *ok goes false when a quotient or digit is not what plain division gives
static uint64_t rekey_one(uint64_t x, const RkArgs &a, const std::vector<uint64_t> &T, bool key64, bool *ok) {
    uint64_t rest = x, y = 0;
    uint32_t left = a.k, row = 0;
    for (uint32_t p = 0; p < a.nparts; p++) {
        const uint32_t nd = left < a.h ? left : a.h;
        uint64_t part;
        if (key64 && p + 1 < a.nparts) {
            uint64_t q = mulhi(rest, a.part_magic), r = rest - q * a.part_div;
            if (r >= a.part_div) { q++; r -= a.part_div; }
            if (q != rest / a.part_div || r != rest % a.part_div) *ok = false;
            part = r; rest = q;
        } else part = rest;
        if (part >> 32) *ok = false;
        for (uint32_t i = 0; i < nd; i++, row += a.base) {
            const uint32_t q = (uint32_t) mulhi(part, a.magic);
            const uint32_t d = (uint32_t) part - q * a.base;
            if (a.base > 1 && (q != part / a.base || d != part % a.base)) *ok = false;
            if (row + d >= T.size()) { *ok = false; return 0; }
            y += T[row + d];
            part = q;
        }
        left -= nd;
    }
    return y;
}

// the same k-mer (digits low first, as letters' indices in `letters`) as a key of an alphabet
static uint64_t key_of(const std::vector<int> &kmer, const RankParams &rp) {
    uint64_t key = 0, pw = 1;
    for (int byte : kmer) { key += (uint64_t) rp.rank_values[byte] * pw; pw *= rp.base; }
    return key;
}

int main() {
    std::mt19937_64 rng(12345);
    uint64_t checked = 0;
    int failures = 0;
    for (uint32_t B = 1; B <= 255 && !failures; B++) {
        // `small`: B letters spread over the bytes; `big`: the same and one more, below, between or above them
        uint8_t small[256] = {}, big[256] = {};
        for (uint32_t i = 0; i < B; i++) small[1 + (i * 254) / B] = 1;
        int extra = (int) (rng() % 256);
        while (small[extra]) extra = (extra + 1) % 256;
        memcpy(big, small, 256); big[extra] = 1;
        uint32_t kmax = 0;
        { unsigned __int128 p = 1; while (kmax < 64 && ((p * (B + 1)) >> 64) == 0) { p *= (B + 1); kmax++; } }
        for (uint32_t k : {kmax, kmax > 1 ? kmax - 1 : 1u, (kmax + 1) / 2, 1u}) {
            if (k == 0) continue;
            const RankParams rs = params_of(small, k), rb = params_of(big, k);
            if (!rk_exact(rs) || !rk_exact(rb)) { printf("B=%u k=%u: not exact\n", B, k); failures++; break; }
            std::vector<uint64_t> up, down;
            const RkArgs au = rk_plan(rs, small, rb, big, up), ad = rk_plan(rb, big, rs, small, down);
            unsigned __int128 top_s = 1, top_b = 1;
            for (uint32_t i = 0; i < k; i++) { top_s *= B; top_b *= B + 1; }
            const bool s64 = top_s > ((unsigned __int128) 1 << 32), b64 = top_b > ((unsigned __int128) 1 << 32);
            std::vector<int> letters;
            for (int b = 0; b < 256; b++) if (small[b]) letters.push_back(b);
            for (int t = 0; t < 64; t++) {
                std::vector<int> kmer(k);
                for (uint32_t i = 0; i < k; i++)                      // random k-mers, and the all-smallest / all-largest ones
                    kmer[i] = t == 0 ? letters.front() : t == 1 ? letters.back() : letters[rng() % letters.size()];
                const uint64_t ks = key_of(kmer, rs), kb = key_of(kmer, rb);
                bool ok = true;
                const uint64_t got_up = rekey_one(ks, au, up, s64, &ok), got_down = rekey_one(kb, ad, down, b64, &ok);
                checked += 2;
                if (!ok || got_up != kb || got_down != ks) {
                    printf("B=%u k=%u: key %" PRIu64 " -> %" PRIu64 " (want %" PRIu64 "), back %" PRIu64 " (want %" PRIu64 ")\n", B, k, ks, got_up, kb, got_down, ks);
                    failures++;
                    break;
                }
            }
        }
    }
    printf("%" PRIu64 " keys re-keyed up and down, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
