// qattn_mla_index_select.hip -- qattn_mla_index_select (include/qattn_mla_index.h): the exact top-k selection of the lightning indexer over
// rows of fp32 logits, gfx950.
//
// WORK ITEM  one workgroup of 16 waves per (slot b, position i) row.
// KEYS       a logit maps to an order-preserving 32-bit key: -0.0 is +0.0, a NaN is -inf, then the sign trick (negative: all bits flipped,
//            else the sign bit set), so a larger logit is a larger unsigned key and equal logits are equal keys.
// SELECT     radix select from the top, 8 bits a pass, 256-bin histograms in LDS.  A pass counts the digit of the keys that match the
//            digits chosen so far; wave 0 walks the bins from the largest digit down to the one where the running count reaches the number
//            still wanted.  After pass 0 the keys of the chosen bin are compacted into LDS when they fit (kCand of them) and passes 1 .. 3
//            read LDS; a bin that overflows -- routine: ReLU makes exact zeros common -- keeps the later passes on the row in global memory
//            (L2).  A wave whose leading lane's digit is shared adds the whole group with ONE LDS atomic: rows of equal values do not
//            serialise.  After four passes the threshold key T and need_eq, the number of keys equal to T still admitted, are exact.
// COMPACT    an ORDERED stream compaction over positions: wave w owns the contiguous segment w of the row.  A first sweep counts, per wave,
//            the keys above T and equal to T; one barrier and a sum over the waves in front give the segment's two prefix sums.  The second
//            sweep places, 64 positions at a time by two ballots, a key above T at (above before) + min(equal before, need_eq) and a key
//            equal to T at the same sum while equal before < need_eq: ascending positions, ties to the lower position, no sort and no
//            atomics on the output.
// LDS (bytes)  histogram 1 024 | candidates 32 768 | wave counts 128 | control 16.
#include "qattn_fp8pv_sweep.h"
#include "qattn_mla_index_select_dev.h"
#include "../../include/qattn_mla_index.h"

using namespace qattn;

namespace {

constexpr int kSelThreads = 1024, kSelWaves = kSelThreads / 64, kCand = QATTN_MLA_INDEX_LDS_CANDIDATES, kUnroll = 8;

struct IndexSelectArgs {
    const float* logits;
    long lsb, lss;   // element strides of the rows
    const int* seqused;
    int* out;        // [B, Sq, topk]
    int Sq, N, topk, causal;
};

// f(position, in range, key) for every position of [0, kend) in rounds of kSelThreads, kUnroll loads in flight; every thread calls f the
// same number of times (f may vote)
template <class F>
__device__ __forceinline__ void for_row_keys(const float* row, int kend, int tid, F f) {
    for (int base = 0; base < kend; base += kSelThreads * kUnroll) {
        float v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int j = base + u * kSelThreads + tid;
            v[u] = j < kend ? row[j] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int j = base + u * kSelThreads + tid;
            f(j, j < kend, order_key(v[u]));
        }
    }
}

// wave 0: the bin, from digit 255 down, where the running count reaches `want` (>= 1, <= the histogram's total).  ctl[0] = the digit,
// ctl[1] = what is still wanted inside the bin, ctl[2] = the bin's count.
__device__ __forceinline__ void find_bin(const unsigned* hist, unsigned want, unsigned* ctl, int lane) {
    unsigned c[4], s = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) { c[q] = hist[255 - 4 * lane - q]; s += c[q]; }
    unsigned incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const unsigned excl = incl - s;
    if (excl < want && want <= incl) {   // exactly one lane
        unsigned r = want - excl;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (r != 0u && r <= c[q]) { ctl[0] = 255u - 4u * lane - q; ctl[1] = r; ctl[2] = c[q]; r = 0u; }
            else if (r != 0u) r -= c[q];
        }
    }
}

// grid = B Sq rows, block = 1024
__global__ __launch_bounds__(kSelThreads) void mla_index_select_kernel(const IndexSelectArgs a) {
    __shared__ unsigned hist[256];
    __shared__ unsigned cand[kCand];
    __shared__ unsigned wcnt[2][kSelWaves];
    __shared__ unsigned ctl[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = (int)(blockIdx.x / (unsigned)a.Sq), pos = (int)(blockIdx.x % (unsigned)a.Sq);
    int L = a.seqused[b];
    L = L < 0 ? 0 : L > a.N ? a.N : L;
    int kend = a.causal ? L - a.Sq + pos + 1 : L;
    kend = kend < 0 ? 0 : kend;
    int* out = a.out + (long)blockIdx.x * a.topk;
    if (kend <= a.topk) {   // every key is selected: no logit is read
        for (int e = tid; e < a.topk; e += kSelThreads) out[e] = e < kend ? e : -1;
        return;
    }
    const float* row = a.logits + (long)b * a.lsb + (long)pos * a.lss;

    // ---- radix select: the topk-th largest key T, and how many keys equal to T are admitted
    unsigned prefix = 0u, want = (unsigned)a.topk, ncand = 0u;
    bool in_lds = false;   // (workgroup-uniform)
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        const unsigned pmask = pass ? 0xffffffffu << (shift + 8) : 0u;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        if (in_lds) {
            for (unsigned base = 0; base < ncand; base += kSelThreads) {
                const unsigned idx = base + tid;
                const unsigned key = idx < ncand ? cand[idx] : 0u;
                hist_add(hist, idx < ncand && (key & pmask) == prefix, (key >> shift) & 255u, lane);
            }
        } else {
            for_row_keys(row, kend, tid, [&](int, bool on, unsigned key) { hist_add(hist, on && (key & pmask) == prefix, (key >> shift) & 255u, lane); });
        }
        __syncthreads();
        if (wave == 0) find_bin(hist, want, ctl, lane);
        __syncthreads();
        const unsigned digit = ctl[0], count = ctl[2];
        want = ctl[1];
        prefix |= digit << shift;
        if (pass == 0 && count <= (unsigned)kCand) {   // the threshold bin fits: its keys move into LDS (in any order: only their values count)
            if (tid == 0) ctl[3] = 0u;
            __syncthreads();
            for_row_keys(row, kend, tid, [&](int, bool on, unsigned key) {
                const bool hit = on && (key >> 24) == digit;
                const unsigned long long m = __ballot(hit);
                if (m == 0ull) return;   // (wave-uniform)
                const int first = __builtin_ctzll(m);
                unsigned at = 0u;
                if (lane == first) at = atomicAdd(&ctl[3], (unsigned)__builtin_popcountll(m));
                at = (unsigned)__builtin_amdgcn_readlane((int)at, first);
                const unsigned slot = at + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
                if (hit && slot < (unsigned)kCand) cand[slot] = key;
            });
            ncand = count;
            in_lds = true;
        }
    }
    const unsigned T = prefix, need_eq = want;   // 1 <= need_eq <= the keys equal to T

    // ---- ordered compaction: wave w owns the positions [s_lo, s_hi), a multiple of 64 long
    const int seg = (int)((((long)kend + kSelWaves * 64 - 1) / (kSelWaves * 64)) * 64);
    const long s_lo_l = (long)wave * seg;
    const int s_lo = s_lo_l < kend ? (int)s_lo_l : kend, s_hi = kend - s_lo < seg ? kend : s_lo + seg;
    unsigned n_gt = 0u, n_eq = 0u;   // (wave-uniform)
    for (int base = s_lo; base < s_hi; base += 64 * kUnroll) {
        float v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int j = base + 64 * u + lane;
            v[u] = j < s_hi ? row[j] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const bool in = base + 64 * u + lane < s_hi;
            const unsigned key = order_key(v[u]);
            n_gt += (unsigned)__builtin_popcountll(__ballot(in && key > T));
            n_eq += (unsigned)__builtin_popcountll(__ballot(in && key == T));
        }
    }
    if (lane == 0) { wcnt[0][wave] = n_gt; wcnt[1][wave] = n_eq; }
    __syncthreads();
    unsigned run_gt = 0u, run_eq = 0u;   // the keys above / equal to T in front of this wave's segment
    for (int w = 0; w < wave; w++) { run_gt += wcnt[0][w]; run_eq += wcnt[1][w]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = s_lo; base < s_hi; base += 64 * kUnroll) {
        float v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int j = base + 64 * u + lane;
            v[u] = j < s_hi ? row[j] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int j = base + 64 * u + lane;
            const bool in = j < s_hi;
            const unsigned key = order_key(v[u]);
            const bool gt = in && key > T, eq = in && key == T;
            const unsigned long long bg = __ballot(gt), be = __ballot(eq);
            const unsigned eq_before = run_eq + (unsigned)__builtin_popcountll(be & below);
            const unsigned at = run_gt + (unsigned)__builtin_popcountll(bg & below) + (eq_before < need_eq ? eq_before : need_eq);
            if ((gt || (eq && eq_before < need_eq)) && at < (unsigned)a.topk) out[at] = j;
            run_gt += (unsigned)__builtin_popcountll(bg);
            run_eq += (unsigned)__builtin_popcountll(be);
        }
    }
}

}  // namespace

extern "C" int qattn_mla_index_select(const float* logits, const long long* logits_strides2, const int* seqused_k, int B, int Sq, int N, int topk,
                                      int is_causal, int* indices, void* stream) {
    if (!logits || !seqused_k || !indices) return QATTN_ERR_INVALID_ARG;
    if (((size_t)logits | (size_t)indices | (size_t)seqused_k) % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Sq <= 0 || N <= 0 || N > (1 << 30) || (long long)B * Sq > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    if (topk <= 0 || topk > QATTN_MLA_SPARSE_MAX_TOPK) return QATTN_ERR_INVALID_ARG;
    if (logits_strides2 && (logits_strides2[0] < 0 || logits_strides2[1] < 0)) return QATTN_ERR_INVALID_ARG;
    IndexSelectArgs a;
    a.logits = logits;
    a.lsb = logits_strides2 ? (long)logits_strides2[0] : (long)Sq * N;
    a.lss = logits_strides2 ? (long)logits_strides2[1] : (long)N;
    a.seqused = seqused_k; a.out = indices;
    a.Sq = Sq; a.N = N; a.topk = topk; a.causal = is_causal ? 1 : 0;
    hipLaunchKernelGGL(mla_index_select_kernel, dim3((unsigned)(B * Sq)), dim3(kSelThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}
