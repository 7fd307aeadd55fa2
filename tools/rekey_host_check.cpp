// rekey_host_check.cpp — the host side of K-rekey (pdl_rekey.h: rank_init_host, rk_exact, rk_change and its rk_plan — digit map,
// table, the two reciprocals) run through every key it is easy to get wrong, as a program of its own so that it can be built with
// the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/rekey_host_check.cpp -o rekey_host_check && ./rekey_host_check
//
// No device is touched: the kernel's arithmetic (rk_items) is repeated here in 128-bit host integers and checked against plain
// division, for alphabets of 1 .. 256 letters at the largest exact k and a few below, growing and shrinking.  The decision is the
// library's own (rk_change, with the rank tables rank_init_host makes, as an append and a removal call it): a letter more or less
// re-keys, the same letters do not, and the first k at which B^k leaves 64 bits is refused by it and by rk_exact alike.  rk_query, the
// decision of a query that brings a letter (option "query_rekey"), gives the same union, the same two plans and the new letter's digit.
#include "../pandelos_amd/csrc/pdl_rekey.h"

#include <cinttypes>
#include <cstring>
#include <random>

static uint64_t mulhi(uint64_t a, uint64_t b) { return (uint64_t) (((unsigned __int128) a * b) >> 64); }

// RankParams of the alphabet `present` as a build makes them
static RankParams params_of(const uint8_t present[256], uint32_t k) {
    RankParams rp;
    uint64_t counters[256];
    for (int b = 0; b < 256; b++) counters[b] = present[b];
    rank_init_host(rp, counters, (int) k);
    return rp;
}
static bool same_params(const RankParams &a, const RankParams &b) {
    return !memcmp(a.rank_values, b.rank_values, 256) && a.last_multiplier == b.last_multiplier && a.base == b.base && a.k == b.k &&
           a.rank_bits == b.rank_bits && a.hash_fallback == b.hash_fallback && a.key_bits == b.key_bits;
}
// `letters` letters at k: rk_exact and rk_change (from one letter fewer, when that is exact) both say "not exact"
static bool refused(uint32_t letters, uint32_t k) {
    uint8_t to[256] = {}, from[256] = {};
    for (uint32_t i = 0; i < letters; i++) to[i] = 1;
    memcpy(from, to, 256); from[letters - 1] = 0;
    if (rk_exact(params_of(to, k))) return false;
    const RankParams rf = params_of(from, k);
    std::vector<uint64_t> table;
    RkChange ch;
    return !rk_exact(rf) || (!rk_change(rf, from, to, table, ch) && !ch.rekey && same_params(ch.rp, params_of(to, k)));
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

static bool same_args(const RkArgs &a, const RkArgs &b) {
    return a.k == b.k && a.base == b.base && a.nparts == b.nparts && a.h == b.h && a.magic == b.magic && a.part_div == b.part_div &&
           a.part_magic == b.part_magic && a.entries == b.entries;
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
    if (!refused(20, 15) || !refused(24, 14) || !refused(2, 64)) { printf("20 letters at k = 15, 24 at k = 14 or 2 at k = 64: not refused\n"); failures++; }
    for (uint32_t B = 1; B <= 255 && !failures; B++) {
        // `small`: B letters spread over the bytes; `big`: the same and one more, below, between or above them
        uint8_t small[256] = {}, big[256] = {};
        for (uint32_t i = 0; i < B; i++) small[1 + (i * 254) / B] = 1;
        int extra = (int) (rng() % 256);
        while (small[extra]) extra = (extra + 1) % 256;
        memcpy(big, small, 256); big[extra] = 1;
        uint32_t kmax = 0;
        { unsigned __int128 p = 1; while (kmax < 64 && ((p * (B + 1)) >> 64) == 0) { p *= (B + 1); kmax++; } }
        {   // the first k at which `big` to the k-th leaves 64 bits: the decision and rk_exact refuse it alike
            uint32_t nb = 0, kout = 1;
            for (int b = 0; b < 256; b++) nb += big[b];
            { unsigned __int128 p = nb; while ((p >> 64) == 0) { p *= nb; kout++; } }
            const RankParams rs = params_of(small, kout), rb = params_of(big, kout);
            std::vector<uint64_t> none;
            RkChange ch;
            if (rk_exact(rb) || (rk_exact(rs) && (rk_change(rs, small, big, none, ch) || ch.rekey || !same_params(ch.rp, rb)))) {
                printf("B=%u k=%u: %u letters taken for exact\n", B, kout, nb); failures++; break;
            }
        }
        for (uint32_t k : {kmax, kmax > 1 ? kmax - 1 : 1u, (kmax + 1) / 2, 1u}) {
            if (k == 0) continue;
            const RankParams rs = params_of(small, k), rb = params_of(big, k);
            if (!rk_exact(rs) || !rk_exact(rb)) { printf("B=%u k=%u: not exact\n", B, k); failures++; break; }
            std::vector<uint64_t> up, down, none;
            RkChange cu, cd, ce;
            // a letter more, a letter fewer: a re-key each way, for the table a build of the other set makes; the same letters: none
            if (!rk_change(rs, small, big, up, cu) || !cu.rekey || !same_params(cu.rp, rb) || memcmp(cu.present, big, 256) ||
                !rk_change(rb, big, small, down, cd) || !cd.rekey || !same_params(cd.rp, rs) || memcmp(cd.present, small, 256)) {
                printf("B=%u k=%u: no re-key between %u and %u letters\n", B, k, B, B + 1); failures++; break;
            }
            if (!rk_change(rb, big, big, none, ce) || ce.rekey || !same_params(ce.rp, rb) || !none.empty()) {
                printf("B=%u k=%u: a re-key for the same %u letters\n", B, k, B + 1); failures++; break;
            }
            const RkArgs &au = cu.args, &ad = cd.args;
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
            // what a query that brings `extra` decides (rk_query, option "query_rekey"): the same union and the same two plans, and
            // the one digit of the union that is the new letter in `absent`; no letter at all is no re-key
            uint32_t bits[8] = {}, no_bits[8] = {};
            bits[extra >> 5] |= 1u << (extra & 31);
            RkQuery rq, rn;
            const uint32_t dx = rb.rank_values[extra];
            bool one_bit = true;
            if (rk_query(rs, small, bits, rq))
                for (uint32_t d = 0; d < 256; d++) one_bit = one_bit && (((rq.absent[d >> 5] >> (d & 31)) & 1u) == (d == dx ? 1u : 0u));
            if (!rq.up.rekey || !same_params(rq.up.rp, rb) || rq.up_table != up || rq.down_table != down || !same_args(rq.down, ad) || !same_args(rq.up.args, au) ||
                !one_bit || !rk_query(rs, small, no_bits, rn) || rn.up.rekey) {
                printf("B=%u k=%u: the query's decision differs from the append's and the removal's\n", B, k); failures++; break;
            }
            checked++;
        }
    }
    {   // 18 letters at k = 15: one more is exact, two more are not — and the query's decision says so
        uint8_t a18[256] = {};
        for (int i = 0; i < 18; i++) a18[65 + i] = 1;
        uint32_t one[8] = {}, two[8] = {};
        one[3] = 1u << 0; two[3] = 3u;                                  // bytes 96, 97
        RkQuery q1, q2;
        const RankParams r18 = params_of(a18, 15);
        if (!rk_exact(r18) || !rk_query(r18, a18, one, q1) || q1.up.rp.base != 19 || rk_query(r18, a18, two, q2) || q2.up.rp.base != 20 || rk_exact(q2.up.rp)) {
            printf("18 letters at k = 15: 19 not taken or 20 taken for exact\n"); failures++;
        }
    }
    printf("%" PRIu64 " keys re-keyed up and down, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
