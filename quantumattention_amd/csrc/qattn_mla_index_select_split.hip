// qattn_mla_index_select_split.hip -- qattn_mla_index_select_split (include/qattn_mla_index_split.h): the exact top-k selection of the
// lightning indexer with ONE ROW CUT ACROSS WORKGROUPS, gfx950.  Bit for bit the output of qattn_mla_index_select.
//
// WORK ITEM  one workgroup of 8 waves per (row, split): the positions [split SEG, min((split + 1) SEG, kend)) of the row, swept kT kU keys a
//            round.  At 256 splits of 131 072 keys a segment is 512 keys: one key a thread, one round.
// LAUNCHES   clear | pass 0 | pass 1 | pass 2 | count | place -- six, whatever the data; the stream's order is the only synchronisation
//            between workgroups: no kernel waits for another workgroup.
// SELECT     radix select from the top on the keys of qattn_mla_index_select_dev.h, digits of 11, 11 and 10 bits.  Pass p builds the digit
//            histogram of its segment's keys that match the digits chosen so far in LDS (hist_add: rows of equal values do not serialise) and
//            adds the non-zero bins to the row's histogram in the workspace with global integer atomics -- sums of integers, the same in any
//            order.  The NEXT launch finds the chosen digit: every workgroup of the row scans the row's histogram of the pass before (8 KiB
//            from L2, four bins a thread from the largest digit down, a wave scan and the wave totals through LDS) for the bin where the
//            running count reaches what is still wanted.  Only the histogram of the LAST pass is scanned: split 0 of a row stores (digits
//            so far, still wanted) in the workspace, a slot per launch, and the launch after it reads the slot of the launch before it -- one
//            writer, readers one launch later.  After pass 2 the threshold key T and need_eq, the keys equal to T still admitted, are
//            exact for any distribution: there is no candidate buffer and no fallback.
// COUNT      scans histogram 2 (T, need_eq; split 0 stores them), then wave w counts the keys above T and equal to T in its sub-segment of
//            WSEG positions: plain stores of the (wave) pairs and of the workgroup's total.
// PLACE      a wave sums the totals of the splits in front of its own and the pairs of the waves in front of it inside its split (a wave
//            reduction over at most 256 + 8 pairs) and runs the ordered compaction of the one-workgroup kernel in its sub-segment: 64
//            positions at a time by two ballots, a key above T at (above before) + min(equal before, need_eq), a key equal to T at the same
//            sum while equal before < need_eq.  The rows with kend <= topk are written here; no launch reads a logit of such a row.
// LDS (bytes)  pass: histogram 8 192 (pass 2: 4 096) | wave totals 32 | control 8.  count: wave totals 32 + 64 | control 8.  place: none.
#include "qattn_fp8pv_sweep.h"
#include "qattn_mla_index_select_dev.h"
#include "../../include/qattn_mla_index_split.h"

using namespace qattn;

namespace {

constexpr int kT = 512, kW = kT / 64, kU = 4, kMaxSplits = QATTN_MLA_INDEX_MAX_SELECT_SPLITS;
constexpr int kHistRow = 2048 + 2048 + 1024;   // the three histograms of a row, in unsigned
constexpr int kStateRow = 8;                   // (digits so far, still wanted) after pass 0, pass 1, pass 2; padded to 32 bytes
constexpr int kCntSplit = 2 * (kW + 1);        // (above T, equal to T) per wave, then the workgroup's total
static_assert(4 * kT == 2048, "find_digit reads four bins a thread");

__host__ __device__ constexpr int pass_shift(int p) { return p == 0 ? 21 : p == 1 ? 10 : 0; }
__host__ __device__ constexpr int pass_bins(int p) { return p == 2 ? 1024 : 2048; }
__host__ __device__ constexpr int pass_offset(int p) { return 2048 * p; }

struct SplitSelectArgs {
    const float* logits;
    long lsb, lss;     // element strides of the rows
    const int* seqused;
    int* out;          // [B, Sq, topk]
    unsigned* hist;    // [B Sq, kHistRow]
    unsigned* state;   // [B Sq, kStateRow]
    unsigned* cnt;     // [B Sq, splits, kCntSplit]
    int Sq, N, topk, causal;
    int seg, wseg;     // positions of a split, of a wave inside it: multiples of 64
};

// grid = (splits, Sq, B)
struct Item {
    const float* row;
    long r;            // the row's number
    int split, kend, lo, hi;
    bool live;         // the row selects (kend > topk) and the segment is not empty
};

__device__ __forceinline__ Item work_item(const SplitSelectArgs& a) {
    Item it;
    const int b = (int)blockIdx.z, pos = (int)blockIdx.y;
    it.split = (int)blockIdx.x;
    it.r = (long)b * a.Sq + pos;
    int L = a.seqused[b];
    L = L < 0 ? 0 : L > a.N ? a.N : L;
    int kend = a.causal ? L - a.Sq + pos + 1 : L;
    it.kend = kend < 0 ? 0 : kend;
    const long lo = (long)it.split * a.seg;
    it.live = it.kend > a.topk && lo < it.kend;
    it.lo = it.live ? (int)lo : it.kend;
    it.hi = it.kend - it.lo < a.seg ? it.kend : it.lo + a.seg;
    it.row = a.logits + (long)b * a.lsb + (long)pos * a.lss;
    return it;
}

// f(in range, key) for every position of [lo, hi) in rounds of kT threads, kU loads in flight; every thread calls f the same number of
// times (f votes)
template <class F>
__device__ __forceinline__ void for_seg_keys(const float* row, int lo, int hi, int tid, F f) {
    for (int base = lo; base < hi; base += kT * kU) {
        float v[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int j = base + u * kT + tid;
            v[u] = j < hi ? row[j] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kU; u++) f(base + u * kT + tid < hi, order_key(v[u]));
    }
}

// the whole workgroup: the bin of g[0 .. bins), from the largest digit down, where the running count reaches `want` (>= 1, <= the
// histogram's total); `want` becomes what is still wanted inside the bin.  Two barriers.
__device__ __forceinline__ unsigned find_digit(const unsigned* g, int bins, unsigned& want, unsigned* wsum, unsigned* ctl, int tid, int lane, int wave) {
    unsigned c[4], s = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int bin = bins - 1 - 4 * tid - q;
        c[q] = bin >= 0 ? g[bin] : 0u;
        s += c[q];
    }
    unsigned incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned front = 0u;
    for (int w = 0; w < wave; w++) front += wsum[w];
    incl += front;
    const unsigned excl = incl - s;
    if (excl < want && want <= incl) {   // exactly one thread
        unsigned r = want - excl;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (r != 0u && r <= c[q]) { ctl[0] = (unsigned)(bins - 1 - 4 * tid - q); ctl[1] = r; r = 0u; }
            else if (r != 0u) r -= c[q];
        }
    }
    __syncthreads();
    want = ctl[1];
    return ctl[0];
}

// the histograms are accumulated into: cleared by the call itself (a kernel, not a memset node: a captured call stays a chain of kernels).
// EVERY row's 20 KiB are cleared, the rows with kend <= topk included, which never touch them: the size follows the shape, not the data --
// 640 KiB at the 32 rows the auto rule splits at the most on 256 CUs, 20 KiB B Sq under an explicit num_splits (the header, WORKSPACE)
__global__ __launch_bounds__(256) void mla_index_split_clear_kernel(uint4* p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <int P>
__global__ __launch_bounds__(kT) void mla_index_split_pass_kernel(const SplitSelectArgs a) {
    constexpr int kBins = pass_bins(P);
    __shared__ unsigned hist[kBins];
    __shared__ unsigned wsum[kW];
    __shared__ unsigned ctl[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Item it = work_item(a);
    if (!it.live) return;   // (workgroup-uniform)
    unsigned* hrow = a.hist + it.r * kHistRow;
    unsigned* st = a.state + it.r * kStateRow;
    for (int bin = tid; bin < kBins; bin += kT) hist[bin] = 0u;
    unsigned prefix = 0u, want = (unsigned)a.topk, pmask = 0u;
    if (P > 0) {
        if (P == 2) { prefix = st[0]; want = st[1]; }
        const unsigned digit = find_digit(hrow + pass_offset(P - 1), pass_bins(P - 1), want, wsum, ctl, tid, lane, wave);
        prefix |= digit << pass_shift(P - 1);
        pmask = 0xffffffffu << pass_shift(P - 1);
        if (it.split == 0 && tid == 0) { st[2 * (P - 1)] = prefix; st[2 * (P - 1) + 1] = want; }
    } else {
        __syncthreads();
    }
    for_seg_keys(it.row, it.lo, it.hi, tid, [&](bool on, unsigned key) {
        hist_add(hist, on && (key & pmask) == prefix, (key >> pass_shift(P)) & (unsigned)(kBins - 1), lane);
    });
    __syncthreads();
    for (int bin = tid; bin < kBins; bin += kT) {
        const unsigned c = hist[bin];
        if (c != 0u) atomicAdd(&hrow[pass_offset(P) + bin], c);
    }
}

// the sub-segment of a wave inside [lo, hi)
__device__ __forceinline__ void wave_range(const SplitSelectArgs& a, const Item& it, int wave, int& w_lo, int& w_hi) {
    const long l = (long)it.lo + (long)wave * a.wseg;
    w_lo = l < it.hi ? (int)l : it.hi;
    w_hi = it.hi - w_lo < a.wseg ? it.hi : w_lo + a.wseg;
}

__global__ __launch_bounds__(kT) void mla_index_split_count_kernel(const SplitSelectArgs a) {
    __shared__ unsigned wsum[kW];
    __shared__ unsigned wcnt[2][kW];
    __shared__ unsigned ctl[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Item it = work_item(a);
    if (!it.live) return;
    unsigned* st = a.state + it.r * kStateRow;
    unsigned want = st[3];
    const unsigned T = st[2] | find_digit(a.hist + it.r * kHistRow + pass_offset(2), pass_bins(2), want, wsum, ctl, tid, lane, wave);
    if (it.split == 0 && tid == 0) { st[4] = T; st[5] = want; }   // want: need_eq, 1 <= need_eq <= the keys equal to T
    int w_lo, w_hi;
    wave_range(a, it, wave, w_lo, w_hi);
    unsigned n_gt = 0u, n_eq = 0u;   // (wave-uniform)
    for (int base = w_lo; base < w_hi; base += 64 * kU) {
        float v[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int j = base + 64 * u + lane;
            v[u] = j < w_hi ? it.row[j] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const bool in = base + 64 * u + lane < w_hi;
            const unsigned key = order_key(v[u]);
            n_gt += (unsigned)__builtin_popcountll(__ballot(in && key > T));
            n_eq += (unsigned)__builtin_popcountll(__ballot(in && key == T));
        }
    }
    unsigned* cnt = a.cnt + (it.r * gridDim.x + it.split) * kCntSplit;
    if (lane == 0) { cnt[2 * wave] = n_gt; cnt[2 * wave + 1] = n_eq; wcnt[0][wave] = n_gt; wcnt[1][wave] = n_eq; }
    __syncthreads();
    if (tid < 2) {
        unsigned s = 0u;
        for (int w = 0; w < kW; w++) s += wcnt[tid][w];
        cnt[2 * kW + tid] = s;
    }
}

__global__ __launch_bounds__(kT) void mla_index_split_place_kernel(const SplitSelectArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Item it = work_item(a);
    int* out = a.out + it.r * a.topk;
    if (it.kend <= a.topk) {   // every key is selected: the splits share the row's topk entries
        for (long e = (long)it.split * kT + tid; e < a.topk; e += (long)gridDim.x * kT) out[e] = e < it.kend ? (int)e : -1;
        return;
    }
    if (!it.live) return;
    const unsigned* st = a.state + it.r * kStateRow;
    const unsigned T = st[4], need_eq = st[5];
    // the keys above / equal to T in front of this wave's sub-segment: the splits in front, then the waves in front inside the split
    const unsigned* cnt = a.cnt + it.r * gridDim.x * kCntSplit;
    unsigned run_gt = 0u, run_eq = 0u;
    for (int k = lane; k < it.split; k += 64) { run_gt += cnt[k * kCntSplit + 2 * kW]; run_eq += cnt[k * kCntSplit + 2 * kW + 1]; }
    if (lane < wave) { run_gt += cnt[it.split * kCntSplit + 2 * lane]; run_eq += cnt[it.split * kCntSplit + 2 * lane + 1]; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { run_gt += __shfl_xor(run_gt, off); run_eq += __shfl_xor(run_eq, off); }
    run_gt = (unsigned)__builtin_amdgcn_readfirstlane((int)run_gt);
    run_eq = (unsigned)__builtin_amdgcn_readfirstlane((int)run_eq);
    int w_lo, w_hi;
    wave_range(a, it, wave, w_lo, w_hi);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = w_lo; base < w_hi; base += 64 * kU) {
        float v[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int j = base + 64 * u + lane;
            v[u] = j < w_hi ? it.row[j] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int j = base + 64 * u + lane;
            const bool in = j < w_hi;
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

struct SplitWorkspace { size_t hist, state, cnt, total; };

SplitWorkspace split_workspace(int B, int Sq, int num_splits) {
    const size_t rows = (size_t)B * Sq;
    SplitWorkspace w;
    w.hist = up256(rows * kHistRow * sizeof(unsigned));
    w.state = up256(rows * kStateRow * sizeof(unsigned));
    w.cnt = up256(rows * num_splits * kCntSplit * sizeof(unsigned));
    w.total = w.hist + w.state + w.cnt;
    return w;
}

constexpr int kAutoMinSeg = QATTN_MLA_INDEX_AUTO_MIN_SEG, kAutoMinKeys = QATTN_MLA_INDEX_AUTO_MIN_KEYS;
constexpr int kAutoMinSplits = QATTN_MLA_INDEX_AUTO_MIN_SPLITS;
static_assert(kAutoMinKeys / kAutoMinSeg >= kAutoMinSplits, "the segment minimum alone never pushes a row under the split minimum");

}  // namespace

extern "C" size_t qattn_mla_index_select_split_workspace_bytes(int B, int Sq, int N, int num_splits) {
    if (B <= 0 || Sq <= 0 || N <= 0 || B > 65535 || Sq > 65535 || num_splits <= 1 || num_splits > kMaxSplits) return 0;
    return split_workspace(B, Sq, num_splits).total;
}

extern "C" int qattn_mla_index_select_auto_splits(int rows, int N, int topk, int num_cus) {
    if (rows <= 0 || N <= 0 || topk <= 0 || num_cus <= 0) return 1;
    if (rows >= num_cus || N < kAutoMinKeys || N <= topk) return 1;
    int s = num_cus / rows;
    if (s > kMaxSplits) s = kMaxSplits;
    if (s > N / kAutoMinSeg) s = N / kAutoMinSeg;   // ceil(N / s) >= kAutoMinSeg
    return s < kAutoMinSplits ? 1 : s;              // fewer splits were measured slower than one workgroup, or no faster, at 16 384 keys
}

extern "C" int qattn_mla_index_select_split(const float* logits, const long long* logits_strides2, const int* seqused_k, int B, int Sq, int N,
                                            int topk, int is_causal, int num_splits, int* indices, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    if (num_splits < 1 || num_splits > kMaxSplits) return QATTN_ERR_INVALID_ARG;
    if (num_splits == 1) return qattn_mla_index_select(logits, logits_strides2, seqused_k, B, Sq, N, topk, is_causal, indices, stream);
    if (!logits || !seqused_k || !indices || !workspace) return QATTN_ERR_INVALID_ARG;
    if (((size_t)logits | (size_t)indices | (size_t)seqused_k) % 4 != 0 || (size_t)workspace % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Sq <= 0 || B > 65535 || Sq > 65535 || N <= 0 || N > (1 << 30)) return QATTN_ERR_INVALID_ARG;
    if (topk <= 0 || topk > QATTN_MLA_SPARSE_MAX_TOPK) return QATTN_ERR_INVALID_ARG;
    if (logits_strides2 && (logits_strides2[0] < 0 || logits_strides2[1] < 0)) return QATTN_ERR_INVALID_ARG;
    const SplitWorkspace w = split_workspace(B, Sq, num_splits);
    if (workspace_bytes < w.total) return QATTN_ERR_INVALID_ARG;
    SplitSelectArgs a;
    a.logits = logits;
    a.lsb = logits_strides2 ? (long)logits_strides2[0] : (long)Sq * N;
    a.lss = logits_strides2 ? (long)logits_strides2[1] : (long)N;
    a.seqused = seqused_k; a.out = indices;
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    a.hist = reinterpret_cast<unsigned*>(base);
    a.state = reinterpret_cast<unsigned*>(base + w.hist);
    a.cnt = reinterpret_cast<unsigned*>(base + w.hist + w.state);
    a.Sq = Sq; a.N = N; a.topk = topk; a.causal = is_causal ? 1 : 0;
    a.seg = ((N + num_splits - 1) / num_splits + 63) / 64 * 64;
    a.wseg = ((a.seg + kW - 1) / kW + 63) / 64 * 64;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)num_splits, (unsigned)Sq, (unsigned)B), block(kT);
    const size_t n16 = (size_t)B * Sq * kHistRow * sizeof(unsigned) / 16;
    const size_t clear_blocks = (n16 + 255) / 256;
    hipLaunchKernelGGL(mla_index_split_clear_kernel, dim3((unsigned)(clear_blocks < 1024 ? clear_blocks : 1024)), dim3(256), 0, st,
                       reinterpret_cast<uint4*>(a.hist), n16);
    hipLaunchKernelGGL(mla_index_split_pass_kernel<0>, grid, block, 0, st, a);
    hipLaunchKernelGGL(mla_index_split_pass_kernel<1>, grid, block, 0, st, a);
    hipLaunchKernelGGL(mla_index_split_pass_kernel<2>, grid, block, 0, st, a);
    hipLaunchKernelGGL(mla_index_split_count_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(mla_index_split_place_kernel, grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

extern "C" size_t qattn_fp8_mla_index_topk_split_workspace_bytes(int B, int Sq, int max_seqlen_k, int select_splits, int own_logits) {
    const size_t rows = own_logits ? 0 : qattn_fp8_mla_index_workspace_bytes(B, Sq, max_seqlen_k);
    return rows + qattn_mla_index_select_split_workspace_bytes(B, Sq, max_seqlen_k, select_splits);
}

extern "C" int qattn_fp8_mla_index_topk_split(const void* q16, int in_fmt, const long long* q_strides3, const float* weights,
                                              const long long* w_strides2, const void* pool, const int* block_table, long long table_stride,
                                              int num_pages, int page_size, int max_pages, const float* scale, const int* seqused_k, int B,
                                              int Hi, int Sq, int max_seqlen_k, int topk, int fp8_fmt, int is_causal, int select_splits,
                                              int* indices, float* logits, void* q8, float* scale_q, void* workspace, size_t workspace_bytes,
                                              void* stream) {
    if (!indices || (size_t)indices % 4 != 0 || (size_t)workspace % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (topk <= 0 || topk > QATTN_MLA_SPARSE_MAX_TOPK || select_splits < 1 || select_splits > kMaxSplits) return QATTN_ERR_INVALID_ARG;
    if (select_splits > 1 && (B <= 0 || Sq <= 0 || B > 65535 || Sq > 65535)) return QATTN_ERR_INVALID_ARG;
    const size_t rows_bytes = logits ? 0 : qattn_fp8_mla_index_workspace_bytes(B, Sq, max_seqlen_k);
    const size_t sel_bytes = qattn_mla_index_select_split_workspace_bytes(B, Sq, max_seqlen_k, select_splits);
    if ((!logits && rows_bytes == 0) || (select_splits > 1 && sel_bytes == 0)) return QATTN_ERR_INVALID_ARG;
    if (rows_bytes + sel_bytes > 0 && (!workspace || workspace_bytes < rows_bytes + sel_bytes)) return QATTN_ERR_INVALID_ARG;
    float* rows = logits ? logits : reinterpret_cast<float*>(workspace);
    const int rc = qattn_fp8_mla_index_scores(q16, in_fmt, q_strides3, weights, w_strides2, pool, block_table, table_stride, num_pages, page_size,
                                              max_pages, scale, seqused_k, B, Hi, Sq, max_seqlen_k, fp8_fmt, is_causal, rows, nullptr,
                                              logits != nullptr, q8, scale_q, stream);
    if (rc != QATTN_OK) return rc;
    return qattn_mla_index_select_split(rows, nullptr, seqused_k, B, Sq, max_seqlen_k, topk, is_causal, select_splits, indices,
                                        reinterpret_cast<unsigned char*>(workspace) + rows_bytes, sel_bytes, stream);
}
