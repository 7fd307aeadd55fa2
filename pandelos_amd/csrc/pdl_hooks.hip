// pdl_hooks.hip — test hooks: the three generic device primitives (scan_and_apply, pdl_scan.h; pdl_radix_offsets and
// pdl_sort_pairs, pdl_sort.h; pdl_merge_streams, pdl_append.h) on a caller's device buffers, so that a test can hold each of
// them against numpy at the sizes where they change their code path (tests/primitive_cases.py, tests/test_gpu_primitives.py).
// The primitives are called as they are; which form runs follows the context's options onepass_scan, lean_radix and lean_records.
//
// Every hook: the lock and `guarded` like every other entry point; the context's stream, waited for before the return (as
// pdl_copy_device does); PDL_ERR_ARGUMENT for a NULL where a pointer is needed or a width that is not instantiated, then
// PDL_ERR_STATE on a context that holds a build (or a multi-GPU build under way) — scan_tmp, sort_tmp, the look-back words and
// the control block, which the hooks grow, are the build's there.  A fresh context gets the control block pdl_families_of_edges
// gives it.
#include "pdl_sort.h"
#include "pdl_append.h"

namespace {

struct HookFlag {
    const uint32_t *flags;
    __device__ uint32_t operator()(uint64_t i) const { return flags[i]; }
};
struct HookApply {
    uint32_t *prefix, *seen;
    __device__ void operator()(uint64_t i, uint32_t flag, uint32_t p) const { prefix[i] = p; seen[i] = flag; }
};
// the two-phase protocol: load() reads the element's flag again from memory — at the index the kernel hands it, clamped below
// the count for the lanes past it — and store() sets the top bit of seen[i] where the two differ (flags are below 2^31)
struct HookApplyTwoPhase {
    uint32_t *prefix, *seen;
    const uint32_t *flags;
    struct Loaded { uint32_t flag; };
    __device__ Loaded load(uint64_t i, uint32_t) const { return Loaded{flags[i]}; }
    __device__ void store(uint64_t i, uint32_t flag, uint32_t p, Loaded v) const { prefix[i] = p; seen[i] = flag | (v.flag != flag ? 0x80000000u : 0u); }
};

template <class Body>
int hook(pdl_ctx *c, const char *who, bool bad_argument, Body &&body) {
    if (!c) return PDL_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(c->mu);
    return guarded(c, [&]() -> int {
        if (bad_argument) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: a NULL pointer, or a width or bit range the primitive is not built for", who);
        if (c->preprocessed || c->dist_stage != DistStage::none)
            PDL_FAIL(PDL_ERR_STATE, "%s: the context holds a build, whose work buffers the hook would grow (use a context without one)", who);
        PDL_HIP(hipSetDevice(c->device));
        pdl_ctl_ready(c);
        body();
        PDL_HIP(hipStreamSynchronize(c->stream));
        return PDL_OK;
    });
}

template <class KeyT, class ValT>
void hook_sort(pdl_ctx *c, void *keys_a, void *keys_b, void *vals_a, void *vals_b, uint64_t n, uint32_t end_bit, bool iota_values, const uint64_t *d_n,
               uint32_t begin_bit, bool keys_below_end_bit, bool filed, int *out_result_in_b) {
    KeyT *ki = static_cast<KeyT *>(keys_a), *ko = static_cast<KeyT *>(keys_b);
    ValT *vi = static_cast<ValT *>(vals_a), *vo = static_cast<ValT *>(vals_b);
    pdl_sort_pairs<KeyT, ValT>(c, ki, ko, vi, vo, n, end_bit, iota_values, d_n, begin_bit, keys_below_end_bit, filed);
    *out_result_in_b = static_cast<void *>(ko) == keys_b ? 1 : 0;
}

}  // namespace

extern "C" {

int pdl_test_scan(pdl_ctx *c, const uint32_t *d_flags, uint64_t n_bound, const uint64_t *d_n, uint32_t *d_prefix, uint32_t *d_seen_flag, int two_phase,
                  uint64_t *d_total, uint64_t *d_total2) {
    return hook(c, "pdl_test_scan", !d_total || (n_bound && (!d_flags || !d_prefix || !d_seen_flag)), [&] {
        if (two_phase) scan_and_apply(c, n_bound, HookFlag{d_flags}, HookApplyTwoPhase{d_prefix, d_seen_flag, d_flags}, d_total, d_total2, d_n);
        else scan_and_apply(c, n_bound, HookFlag{d_flags}, HookApply{d_prefix, d_seen_flag}, d_total, d_total2, d_n);
        if (c->opt_onepass_scan) {                       // the look-back error word, as a stage reads it
            PinRead rd(c);
            const uint32_t *e = lookback_error_word(c, rd);
            rd.sync();
            lookback_check(c, e);
        }
    });
}

int pdl_test_radix_offsets(pdl_ctx *c, const uint32_t *d_counts, uint32_t *d_offs, uint32_t n_tiles, uint64_t *d_total, uint32_t *d_digit_total,
                           int *out_lean) {
    return hook(c, "pdl_test_radix_offsets", !d_counts || !d_offs || !d_total || !d_digit_total || !out_lean, [&] {
        if ((uint64_t) n_tiles * PDL_RADIX_TILE >= 0xfffff000ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_test_radix_offsets: %u tiles are more than a pass can have", n_tiles);
        *out_lean = pdl_radix_offsets(c, d_counts, d_offs, n_tiles, d_total, d_digit_total) ? 1 : 0;
    });
}

int pdl_test_sort_pairs(pdl_ctx *c, uint32_t key_bytes, uint32_t val_bytes, void *d_keys_a, void *d_keys_b, void *d_vals_a, void *d_vals_b, uint64_t n,
                        uint32_t end_bit, int iota_values, const uint64_t *d_n, uint32_t begin_bit, int keys_below_end_bit, const uint32_t *d_first_counts,
                        int *out_result_in_b, uint64_t *out_total) {
    const bool widths = (key_bytes == 4 && val_bytes == 4) || (key_bytes == 8 && val_bytes == 4) || (key_bytes == 4 && val_bytes == 8);
    const bool null = !out_result_in_b || !out_total || (n && (!d_keys_a || !d_keys_b || !d_vals_a || !d_vals_b));
    return hook(c, "pdl_test_sort_pairs", null || !widths || begin_bit % 8 != 0, [&] {
        // (all ones where no pass runs: the word shows what the last pass left, and that one did)
        uint64_t *d_total = c->scalars.as<uint64_t>() + PDL_CTL_SCAN_TOTAL;
        PDL_HIP(hipMemsetAsync(d_total, 0xff, sizeof(uint64_t), c->stream));
        if (d_first_counts && n) {
            c->sort_tmp.alloc(pdl_radix_tmp_bytes(n));
            const size_t table = (size_t) PDL_RADIX_BINS * ((n + PDL_RADIX_TILE - 1) / PDL_RADIX_TILE) * sizeof(uint32_t);
            PDL_HIP(hipMemcpyAsync(c->sort_tmp.p, d_first_counts, table, hipMemcpyDeviceToDevice, c->stream));
        }
        const bool filed = d_first_counts != nullptr;
        *out_result_in_b = 0;
        if (key_bytes == 8) hook_sort<uint64_t, uint32_t>(c, d_keys_a, d_keys_b, d_vals_a, d_vals_b, n, end_bit, iota_values != 0, d_n, begin_bit, keys_below_end_bit != 0, filed, out_result_in_b);
        else if (val_bytes == 8) hook_sort<uint32_t, unsigned long long>(c, d_keys_a, d_keys_b, d_vals_a, d_vals_b, n, end_bit, iota_values != 0, d_n, begin_bit, keys_below_end_bit != 0, filed, out_result_in_b);
        else hook_sort<uint32_t, uint32_t>(c, d_keys_a, d_keys_b, d_vals_a, d_vals_b, n, end_bit, iota_values != 0, d_n, begin_bit, keys_below_end_bit != 0, filed, out_result_in_b);
        PDL_HIP(hipMemcpyAsync(out_total, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    });
}

int pdl_test_merge(pdl_ctx *c, uint32_t key_bytes, const void *d_a_keys, const uint32_t *d_a_vals, uint32_t na, const void *d_b_keys, const uint32_t *d_b_vals,
                   uint32_t nb, uint32_t b_val_add, uint64_t mask, void *d_out_keys, uint32_t *d_out_vals) {
    const bool null = (na && (!d_a_keys || !d_a_vals)) || (nb && (!d_b_keys || !d_b_vals)) || ((na || nb) && (!d_out_keys || !d_out_vals));
    return hook(c, "pdl_test_merge", null || (key_bytes != 4 && key_bytes != 8), [&] {
        const uint64_t total = (uint64_t) na + nb;
        if (total >= 0xffffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_test_merge: %llu elements need 64-bit positions", (unsigned long long) total);
        DevBuf split;                                    // the hook's own: freed behind the wait below
        split.alloc(pdl_merge_split_words(total) * sizeof(uint32_t));
        if (key_bytes == 8)
            pdl_merge_streams<uint64_t>(c->stream, static_cast<const uint64_t *>(d_a_keys), d_a_vals, na, static_cast<const uint64_t *>(d_b_keys), d_b_vals, nb,
                                        b_val_add, mask, split.as<uint32_t>(), static_cast<uint64_t *>(d_out_keys), d_out_vals);
        else
            pdl_merge_streams<uint32_t>(c->stream, static_cast<const uint32_t *>(d_a_keys), d_a_vals, na, static_cast<const uint32_t *>(d_b_keys), d_b_vals, nb,
                                        b_val_add, (uint32_t) mask, split.as<uint32_t>(), static_cast<uint32_t *>(d_out_keys), d_out_vals);
        PDL_HIP(hipStreamSynchronize(c->stream));
    });
}

}  // extern "C"
