// kbbh_host_check.cpp — the host helpers of K-bbh and K-place that need no device (pdl_common.h: bbh_cut_blocks, fam_of_label,
// BaseBufs::view, PinBuf's bookkeeping), as a program of its own so that it can be built with the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/kbbh_host_check.cpp -o kbbh_host_check && ./kbbh_host_check
//
// No device is touched: PinBuf::alloc of more than it holds and the uploads themselves need one and are not run here.
#include "../pandelos_amd/csrc/pdl_common.h"

void pdl_set_create_error(const std::string &) {}        // (guarded's, never reached here)

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); failures++; } } while (0)

// bbh_cut_blocks' refusal for these counts ("" when it serves)
static std::string cut(uint64_t t1, uint64_t t2, const std::vector<uint32_t> *picks, const std::vector<uint32_t> &at, uint64_t Z, std::vector<uint64_t> &e1,
                       std::vector<uint64_t> &e2) {
    try { bbh_cut_blocks("check", t1, t2, picks ? picks->data() : nullptr, picks ? at.data() : nullptr, (uint32_t) at.size() - 1, Z, 7, e1, e2); }
    catch (const pdl_error &e) { return e.code == PDL_ERR_DEVICE ? e.msg : "another code: " + e.msg; }
    return "";
}

int main() {
    using V = std::vector<uint64_t>;
    V e1, e2;
    // one block: the totals close the lists
    CHECK(cut(3, 2, nullptr, {0, 10}, 10, e1, e2) == "" && e1 == V({0, 6}) && e2 == V({0, 2}), "one block");
    CHECK(cut(11, 0, nullptr, {0, 10}, 10, e1, e2) == "check: 11 + 0 edge cells of 10 cells", "phase-1 total above Z");
    CHECK(cut(0, 11, nullptr, {0, 10}, 10, e1, e2) == "check: 0 + 11 edge cells of 10 cells", "phase-2 total above Z");
    // four blocks, the third empty, the last two starting at Z: their picks are never read (stale words there)
    const std::vector<uint32_t> at{0, 4, 4, 10, 10};
    std::vector<uint32_t> picks{0, 2, 2, 99, 99, /* phase 2 */ 0, 1, 1, 99, 99};
    CHECK(cut(5, 3, &picks, at, 10, e1, e2) == "" && e1 == V({0, 4, 4, 10, 10}) && e2 == V({0, 1, 1, 3, 3}), "four blocks");
    picks[2] = 1;                    // phase 1 decreases at block 1 -> named with the caller's index of block 0 added
    CHECK(cut(5, 3, &picks, at, 10, e1, e2) == "check: inconsistent edge offsets at block 8", "decreasing offsets: %s", cut(5, 3, &picks, at, 10, e1, e2).c_str());
    picks[2] = 2; picks[6] = 4;      // phase 2 passes its total
    CHECK(cut(5, 3, &picks, at, 10, e1, e2) == "check: inconsistent edge offsets at block 7", "offsets past the total");
    picks[6] = 1; picks[1] = 6;      // phase 1 passes its total
    CHECK(cut(5, 3, &picks, at, 10, e1, e2) == "check: inconsistent edge offsets at block 7", "phase-1 offsets past the total");

    // the family of every label: three families over eight genes, genes 2 and 6 no nodes
    const uint32_t comp[8] = {0, 1, 2, 1, 0, 5, 6, 5}, off[4] = {0, 2, 4, 6}, genes[6] = {0, 4, 1, 3, 5, 7};
    const uint8_t node[8] = {1, 1, 0, 1, 1, 1, 0, 1}, col[3] = {0, 1, 0};
    BaseBufs b;
    fam_of_label(FamView{8, 3, 6, comp, off, genes, node, col}, b.of_label);
    CHECK(b.of_label == std::vector<uint32_t>({0, 1, 0, 0, 0, 2, 0, 0}), "fam_of_label");
    fam_of_label(FamView{0, 0, 0, nullptr, off, nullptr, nullptr, nullptr}, b.of_label);
    CHECK(b.of_label.empty(), "fam_of_label of no gene");
    const uint32_t gen[1] = {0};
    const PlaceBase B = b.view(8, gen, 4);
    CHECK(!B.comp && !B.fam_of_label && B.genome_of == gen && B.N == 8 && B.G == 4, "the view of buffers that hold nothing");

    PinBuf p;                        // what needs no allocation
    p.alloc(0); p.release();
    CHECK(!p.p && !p.bytes, "PinBuf without a need");
    printf("kbbh_host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
