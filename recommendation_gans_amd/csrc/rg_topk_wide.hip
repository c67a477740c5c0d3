// Top-k beyond the register lists (rg_topk_rows_wide, 1 <= k <= RG_TOPK_WIDE_MAX): the first k
// columns of each row in rg_topk_lists.h's total order -- key descending, column ascending, the
// key of a NaN is -inf -- so for k <= 32 the ids are rg_topk_rows' ids.  A sorted list per thread
// does not reach k = 1024; this selects instead of inserting.
//
// One workgroup per row, five passes over the row (re-read from cache after the first):
//   1-4  radix select of the k-th key, 8 bits a pass, most significant first.  Each value maps to
//        an order-preserving 32-bit key (wide_key); a pass histograms one digit of the keys that
//        share the prefix found so far (256 LDS counters), a scan from the top bin finds the bin
//        the k-th key falls in, and k becomes the rank inside that bin.  After four passes the
//        prefix is the threshold key T, and the rank is how many columns with key T are wanted.
//   5    collect.  Every column with key > T takes the next free slot (an LDS counter: their
//        order does not matter, the sort below fixes it).  The columns with key == T are taken
//        lowest column first: the waves split the row into contiguous segments and walk them in
//        order, 64 columns at a time; a ballot gives each tied column its position within the
//        wave, and a wave keeps at most the first `need` of its segment in an LDS staging list.
//        The lists are then concatenated in wave order up to `need`.  No tied column is placed
//        by an atomic, so thousands of ties (excluded -inf columns, scores saturated at 1.0) give
//        the same k columns whatever the waves' schedule.
// The k survivors are composite 64-bit keys (key << 32 | ~column), all distinct; a bitonic sort in
// LDS puts them in rank order.  Integer counts and compares only: the result is deterministic.
#include <climits>

#include "rg_common.h"
#include "rg_topk_lists.h"

namespace rg {
namespace {

constexpr int kWideThreads = 256;
constexpr int kWideWaves = kWideThreads / kWave;
constexpr int kWideMax = RG_TOPK_WIDE_MAX;
constexpr int kWideBins = 256;            // 8-bit digits: one bin per thread in the scan
constexpr int kWideUnroll = 4;            // loads in flight per thread and pass
static_assert(kWideBins == kWideThreads, "the bin scan gives every thread one bin");
static_assert((kWideMax & (kWideMax - 1)) == 0, "the bitonic sort runs on a power of two");

// Order-preserving key: a > b as floats (by rg_topk_lists.h's key_of) iff wide_key(a) > wide_key(b),
// equal iff equal.  Integer operations only.  Every NaN bit pattern becomes -inf, and -0.0 becomes
// +0.0: better() compares them equal, a raw bit pattern would rank them apart.  The smallest key is
// -inf's 0x007fffff, so 0 is free as the sort's padding.
__device__ __forceinline__ uint32_t wide_key(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0xff800000u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t wide_pack(uint32_t key, int col) {
    return ((uint64_t)key << 32) | (uint32_t)~(uint32_t)col;
}

__global__ __launch_bounds__(kWideThreads) void topk_wide_kernel(const float *__restrict__ scores, int64_t cols,
                                                                 int64_t ld, int k, int32_t *__restrict__ out_idx,
                                                                 float *__restrict__ out_val) {
    __shared__ uint64_t comp[kWideMax];                 // the survivors, then sorted
    __shared__ int stage[kWideWaves][kWideMax];         // each wave's first tied columns, in order
    __shared__ uint32_t hist[kWideBins];
    __shared__ uint32_t wsum[kWideWaves];
    __shared__ int s_neq[kWideWaves];
    __shared__ uint32_t s_prefix, s_need, s_above;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const float *row = scores + (int64_t)blockIdx.x * ld;
    int n = 2;                                          // sorted entries: a power of two >= k
    while (n < k) n <<= 1;
    // an entry that no pass fills (none, unless the block changes under the kernel) stays 0:
    // the id -1, which is never used as an index below
    for (int j = tid; j < n; j += kWideThreads) comp[j] = 0;
    if (tid == 0) s_above = 0;

    // ---- passes 1-4: the k-th key
    uint32_t prefix = 0, need = (uint32_t)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        hist[tid] = 0;
        __syncthreads();
        // equal digits in a row are counted in a register and added once: scores of one
        // magnitude share their leading digits, and every lane would queue on one counter
        int cur = 0;
        uint32_t run = 0;
        for (int64_t c0 = tid; c0 < cols; c0 += kWideUnroll * kWideThreads) {
            float x[kWideUnroll];
#pragma unroll
            for (int j = 0; j < kWideUnroll; ++j) {
                const int64_t c = c0 + j * kWideThreads;
                x[j] = c < cols ? row[c] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < kWideUnroll; ++j) {
                const uint32_t key = wide_key(x[j]);
                if (c0 + j * kWideThreads < cols && (key & mask) == prefix) {
                    const int d = (int)((key >> shift) & (kWideBins - 1));
                    if (d == cur) {
                        ++run;
                    } else {
                        if (run) atomicAdd(&hist[cur], run);
                        cur = d;
                        run = 1;
                    }
                }
            }
        }
        if (run) atomicAdd(&hist[cur], run);
        __syncthreads();
        // thread t holds bin 255 - t: the inclusive scan over t counts the keys in its bin and above
        const int bin = kWideBins - 1 - tid;
        const uint32_t h = hist[bin];
        uint32_t incl = h;
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == kWave - 1) wsum[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += wsum[w];
        // exactly one bin: need <= the count of keys under the prefix (k <= cols at the start)
        if (incl - h < need && need <= incl) {
            s_prefix = prefix | ((uint32_t)bin << shift);
            s_need = need - (incl - h);
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
    }
    const uint32_t T = prefix;                          // need columns with key T, k - need above it
    const int n_above = k - (int)need;

    // ---- pass 5: collect
    const int64_t seg = (cols + kWideWaves * kWave - 1) / (kWideWaves * kWave) * kWave;
    const int64_t lo = (int64_t)wave * seg, hi = lo + seg < cols ? lo + seg : cols;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    int64_t n_eq = 0;                                   // wave-uniform: tied columns seen so far
    for (int64_t c0 = lo; c0 < hi; c0 += kWideUnroll * kWave) {
        float x[kWideUnroll];
#pragma unroll
        for (int j = 0; j < kWideUnroll; ++j) {
            const int64_t c = c0 + j * kWave + lane;
            x[j] = c < hi ? row[c] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < kWideUnroll; ++j) {
            const int64_t c = c0 + j * kWave + lane;
            const uint32_t key = wide_key(x[j]);
            if (c < hi && key > T) {
                const uint32_t slot = atomicAdd(&s_above, 1u);
                if (slot < (uint32_t)n_above) comp[slot] = wide_pack(key, (int)c);
            }
            const bool eq = c < hi && key == T;
            const uint64_t m = __ballot(eq);
            const int64_t pos = n_eq + __popcll(m & below);
            if (eq && pos < (int64_t)need) stage[wave][pos] = (int)c;
            n_eq += __popcll(m);
        }
    }
    if (lane == 0) s_neq[wave] = (int)(n_eq < (int64_t)need ? n_eq : (int64_t)need);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < kWideWaves; ++w) {
        const int cnt = s_neq[w];
        for (int j = tid; j < cnt && base + j < (int)need; j += kWideThreads)
            comp[n_above + base + j] = wide_pack(T, stage[w][j]);
        base += cnt;
    }
    __syncthreads();

    // ---- rank order: bitonic sort, descending
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < n / 2; t += kWideThreads) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t a = comp[i], b = comp[j];
                if ((a < b) == ((i & size) == 0)) {
                    comp[i] = b;
                    comp[j] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += kWideThreads) {
        const int col = (int)~(uint32_t)comp[j];
        out_idx[(int64_t)blockIdx.x * k + j] = col;
        if (out_val) out_val[(int64_t)blockIdx.x * k + j] = col >= 0 && col < cols ? row[col] : NAN;
    }
}

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int rg_topk_rows_wide(void *stream, const float *scores, int64_t rows, int64_t cols, int64_t ld,
                                 int32_t k, int32_t *out_idx, float *out_val) {
    if (!scores || !out_idx) return fail_arg("rg_topk_rows_wide: null argument");
    if (rows < 0 || cols < 1 || ld < cols) return fail_arg("rg_topk_rows_wide: bad shape");
    if (cols > INT_MAX) return fail_arg("rg_topk_rows_wide: cols must fit int32");
    if (rows > INT_MAX) return fail_arg("rg_topk_rows_wide: too many rows for one launch");
    if (k < 1 || k > kWideMax || k > cols)
        return fail_arg("rg_topk_rows_wide: k must be in [1, min(" + std::to_string(kWideMax) + ", cols)]");
    if (rows == 0) return RG_OK;
    hipLaunchKernelGGL(topk_wide_kernel, dim3((unsigned)rows), dim3(kWideThreads), 0, (hipStream_t)stream, scores,
                       cols, ld, (int)k, out_idx, out_val);
    return check_launch("rg_topk_rows_wide");
}
