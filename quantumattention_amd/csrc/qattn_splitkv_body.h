// qattn_splitkv_body.h -- the BODY of the split-KV sweep kernel, included inside the two kernel definitions of qattn_splitkv_attn.h (no include
// guard: it is text, not declarations).  QATTN_SKV_PAGED selects where a head's 64-key chunks are fetched from: 0, the contiguous images
// (a.k8 / a.v8 + the head's offset, chunk c is chunk c) -- statement for statement the kernel qattn_splitkv_fp8.hip held before the paged
// entry existed, so that its device code stays what it was; 1, the pools through the block table `pg` (include/qattn_paged.h).  A body
// shared as text, not as an inlined function: wrapped in a function the compiler's inlining and register allocation came out differently
// for the contiguous kernels (profiles/paged/code_objects_vs_parent.log).
// QATTN_SKV_VARQ (with QATTN_SKV_PAGED; include/qattn_paged_varlen.h) selects where a workgroup's QUERY rows live: 0, the dense
// [B, Hq, Sq, D] tensors, every sequence with a.Sq queries; 1, packed tensors [total_q, Hq, D] cut by cu_seqlens_q (`vq`, SkvVarq): the
// workgroup finds its (sequence, tile) by the binary search of qattn_varlen_tile.h on the packed-row starts G cu[i], and the sequence's
// own Sq_i stands wherever the dense kernels read a.Sq.  The names that differ are macros (SKV_SQ, SKV_ROWS, SKV_QROW, SKV_QROW0, SKV_OROW,
// SKV_LROW), so that with the switch off the text the compiler sees is token for token what it was
// (profiles/paged_varlen/code_objects_vs_parent.log).
// QATTN_SKV_WINDOW (include/qattn_splitkv_window.h) puts a sliding window (wn, SkvWindow: left / right, -1 = unbounded) where a.causal
// stands: 0, the text above, token for token (profiles/splitkv_window/code_objects_vs_parent.log); 1, the split plan cuts the sequence's
// interval [lo_i, L) instead of [0, L), the tile's trip range gets a lower end klo, the token mask a lower edge, and the V bytes of the
// keys below lo_i that share its 64-key chunk are zeroed in LDS (skv_zero_v_head).  a.causal is then not read.  The edge offsets win_lo /
// win_hi are attn_vfp8_window_kernel's, clamped exactly so that every sum below stays in 32 bits, and padding rows get that kernel's
// masks: with one split, G = 1 and contiguous K / V the wave-mates, chunks and masks are its own.
// QATTN_SKV_SINK (with QATTN_SKV_WINDOW; include/qattn_sinks.h) adds a learned per-head logit `sn.sink[head]` (natural-log units of the
// scaled scores) to the softmax denominator: 0, the text above, token for token (profiles/sinks/code_objects_vs_parent.log); 1, a call
// with ONE split folds the sink into the epilogue -- l' = l + exp2(sink log2e - (m c - kPShift)), loaded after the sweep loop so that it
// lives in no register across it -- and a tile without a key stores zero rows with LSE = sink.  With more splits the partials are written
// WITHOUT the sink (the statements of the switch-off text): it enters the last launch of the merge chain.  sink = -inf adds 0.0f to l: the
// row's bits are the window kernel's.  sink = +inf or NaN: the head's rows are NaN.
// QATTN_SKV_TREE (with QATTN_SKV_PAGED and QATTN_SKV_VARQ, without QATTN_SKV_WINDOW; include/qattn_paged_varlen_tree.h) puts a draft tree
// over the causal rule: 0, the text above, token for token (profiles/tree/code_objects_vs_parent.log); 1, a sequence with Sq_i <= 64 queries
// holds its draft tokens in its last Sq_i keys, and the row of position p attends key j >= max(delta, 0) only if bit j - delta of the
// token's 64-bit word `tr.mask[token]` is set -- one load per lane before the sweep loop, applied in the edge branch below, which is then
// entered for every chunk that holds a key >= delta.  The split plan, khi, c_first, n_wg, the ring and the epilogue are the causal text:
// a word with the bits 0 .. p set gives the causal kernel's bits.  (The entry is causal: its driver sets a.causal.)
// QATTN_SKV_TREE with QATTN_SKV_WINDOW (and, optionally, QATTN_SKV_SINK; include/qattn_paged_varlen_tree_window.h) puts the draft tree over
// the WINDOW text instead, for windows (left, 0) with left = -1 or left >= 63: a draft token of a sequence with Sq_i <= 64 queries sits at
// sequence position delta + DEPTH, depth = the set bits of its word below its own index, so wherever the window text takes a row's
// position for the window's LOWER edge (lo_l, and through smin / smax klo and edge_lo) this text takes the row's depth; the upper edge
// (hi_l, khi, edge) stays by position, as the tree text has it.  The least and the greatest depth of the tile's valid rows (dmin, dmax)
// are reduced per wave from the tile's words BEFORE the plan's `keys` count and the `sel` return, so that a chain -- depth = position --
// reproduces the window kernel's klo, keys, selection and trip range.  With left >= 63 every lo_l <= max(delta, 0): the lower edge never
// cuts a draft key, so one comparison serves committed and draft keys alike.  A sequence with more than 64 queries reads no word and is
// the window text (depth = position).  Both switches off the combination: the text above, token for token
// (profiles/tree_window/code_objects_vs_parent.log).
// QATTN_SKV_SOFTCAP (with QATTN_SKV_WINDOW, without QATTN_SKV_SINK and QATTN_SKV_TREE; include/qattn_softcap.h) caps the scaled scores:
// y = softcap tanh(x / softcap).  0: the text above, token for token (profiles/softcap/code_objects_vs_parent.log); 1, every
// raw score s of a chunk is replaced by t = tanh(s kin) in [-1, 1] between sw.qk and the token mask -- on every chunk, before the mask, so
// that a masked key is -inf and never exp(-softcap) -- with the row's kin = sm_scale scale_q scale_k / softcap, and the sweep is handed
// c = softcap log2e in sm_log2e scale_q scale_k's place: m_run, the rescale limit, the two-term split and the LSE epilogue work on t as
// they work on raw scores.  tanh is 1 - 2 / (1 + 2^(2 log2e u)): one v_exp_f32 and one v_rcp_f32 per score, +-1 at large |u| without a
// NaN, NaN for a NaN score.  sc.kin2 carries 2 log2e sm_scale / softcap, so the exponent is one multiply away from the raw score.
// In scope: template parameters D, FMT, BYTE; arguments a (SkvAttn), two, sel, -- paged -- pg (SkvPages), -- packed queries -- vq,
// -- window -- wn, -- sink -- sn (SkvSink), -- tree -- tr (SkvTree) and -- soft cap -- sc (SkvSoftcap).
#if QATTN_SKV_VARQ
#define SKV_SQ Sq_i
#define SKV_ROWS rows_i
#define SKV_QROW qrow     // this lane's row of q8, in rows of D bytes
#define SKV_QROW0 qrow0   // ... and the first row of the kv head's group: what a padding lane reads
#define SKV_OROW orow     // row of the token-major [total_q, Hq] space: out, partial_o
#define SKV_LROW lrow     // row of the head-major [Hq, total_q] space: lse, row_path, partial_lse, partial_path
#define SKV_HEAD head     // this lane's query head: the sink's index
#else
#define SKV_SQ a.Sq
#define SKV_ROWS a.rows
#define SKV_QROW grow
#define SKV_QROW0 ((long)kvh * a.rows)
#define SKV_OROW grow
#define SKV_LROW grow
#define SKV_HEAD ((kvh % a.Hkv) * a.G + g)
#endif
    constexpr int CH = 64 * D, MB = D / 32, KS = D / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    FpvSweep<D, FMT, BYTE> sw(smem);
    const int lane = sw.lane, wave = sw.wave, ql = sw.ql, hh = sw.hh;

    // block -> (kv head b Hkv + hkv, tile, split): the splits of a tile are neighbours, the tiles of a kv head follow each other.
    // (Handing each XCD a contiguous range of kv heads, as the other launchers do, was measured and moved no time: not kept.)
    const int bid = blockIdx.x, per_head = a.ntile * a.ns;
#if QATTN_SKV_VARQ
    // a.ntile = B + ceil(G total_q / 128) tile slots per kv head; slot jt belongs to the largest sequence i with i + floor(G start_i / 128)
    // <= jt (strictly increasing in i: consecutive values differ by at least ceil(G Sq_i / 128)) as its tile jt - that -- or to no tile.
    // Every extent is clamped (include/qattn_varlen.h), so no table content moves a row out of [0, total_q).
    const int hkv = bid / per_head, rest = bid % per_head;
    const int s = rest % a.ns, jt = rest / a.ns;
    int seq = 0, seq_hi = vq.B - 1;
    while (seq < seq_hi) {   // (workgroup-uniform)
        const int mid = (seq + seq_hi + 1) >> 1;
        const int st = clampi(__builtin_amdgcn_readfirstlane(vq.cu[mid]), 0, vq.total_q);
        if (mid + (a.G * st) / kFpvTile <= jt) seq = mid;
        else seq_hi = mid - 1;
    }
    const int q_start = clampi(__builtin_amdgcn_readfirstlane(vq.cu[seq]), 0, vq.total_q);
    const int Sq_i = clampi(__builtin_amdgcn_readfirstlane(vq.cu[seq + 1]), q_start, vq.total_q) - q_start;
    const int rows_i = a.G * Sq_i;
    const int tile = jt - (seq + (a.G * q_start) / kFpvTile);
    if (tile < 0 || tile > ((rows_i - 1) >> 7)) return;   // before any other memory is touched (rows_i = 0: -1 >> 7 = -1)
    const int kvh = seq * a.Hkv + hkv;                    // (sequence, kv head): scales, seqused_k and the table's row as in the dense kernels
#else
    const int kvh = bid / per_head, rest = bid % per_head;
    const int s = rest % a.ns, tile = rest / a.ns;
#endif
    int L = a.Skv;
    if (a.used) L = clampi(__builtin_amdgcn_readfirstlane(a.used[kvh / a.Hkv]), 0, a.Skv);
    // the split plan (workgroup-uniform, as everything down to the row numbers)
#if QATTN_SKV_WINDOW
    // position p attends the keys j with win_lo <= j - p <= win_hi.  j - p lies in (-Sq, L): an offset clamped to [-Sq, L] masks the same
    // keys as the exact one.  The plan cuts the key blocks of the sequence's interval [lo_i, L): a function of (L, Sq, left, ns) alone
    const long delta = (long)L - SKV_SQ;
    auto clampl = [](long x, long lo, long hi) -> int { return (int)(x < lo ? lo : x > hi ? hi : x); };
    const int win_lo = wn.left < 0 ? -SKV_SQ : clampl(delta - wn.left, -(long)SKV_SQ, L);
    const int win_hi = wn.right < 0 ? L : clampl(delta + wn.right, -(long)SKV_SQ - 1, L);
    const int lo_i = wn.left < 0 ? 0 : max(win_lo, 0);
    const int kb0 = lo_i >> 7;
    const int nkb = ((L + 127) >> 7) - kb0, per = (nkb + a.ns - 1) / a.ns;
    const int k_begin = 128 * (kb0 + s * per), k_end = min(128 * (kb0 + (s + 1) * per), L);
#else
    const int nkb = (L + 127) >> 7, per = (nkb + a.ns - 1) / a.ns;
    const int k_begin = 128 * s * per, k_end = min(128 * (s + 1) * per, L);
#endif
    const int r_first = tile * kFpvTile, r_last = min(r_first + kFpvTile, SKV_ROWS) - 1;
    // positions of the tile's valid rows: [smin, smax] (a tile that crosses a head boundary holds a last and a first position)
    const int g_first = r_first / SKV_SQ, g_last = r_last / SKV_SQ;
    const int smin = g_first != g_last ? 0 : r_first - g_first * SKV_SQ, smax = g_first != g_last ? SKV_SQ - 1 : r_last - g_first * SKV_SQ;
#if QATTN_SKV_WINDOW && QATTN_SKV_TREE
    // depths of the tile's valid rows: [dmin, dmax].  Every wave reduces the tile's 128 words by itself -- two per lane, no LDS beside the
    // ring, no barrier -- and the result is workgroup-uniform.  Row rr of the kv head's packed rows is position rr % Sq_i of the sequence
    // (any head: the word is the token's); q_start + position < q_start + Sq_i <= total_q.  A sequence with more than 64 queries: positions
    int dmin = smin, dmax = smax;
    if (SKV_SQ <= 64) {
        int d_lo = INT_MAX, d_hi = -1;
#pragma unroll
        for (int i = 0; i < kFpvTile; i += 64) {
            const int rr = r_first + i + lane;
            if (rr <= r_last) {
                const int pp = rr % SKV_SQ;
                const int d = __builtin_popcountll(tr.mask[q_start + pp] & ((1ull << pp) - 1ull));
                d_lo = min(d_lo, d);
                d_hi = max(d_hi, d);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            d_lo = min(d_lo, __shfl_xor(d_lo, off));
            d_hi = max(d_hi, __shfl_xor(d_hi, off));
        }
        dmin = __builtin_amdgcn_readfirstlane(d_lo);
        dmax = __builtin_amdgcn_readfirstlane(d_hi);
    }
    // [klo, khi]: the keys of the split that the tile's valid rows attend -- the lower end by depth, the upper end by position
    const int klo = max(k_begin, wn.left < 0 ? 0 : clampl((long)dmin + win_lo, 0, L));
    const int khi = min(k_end - 1, clampl((long)smax + win_hi, -1, L - 1));
    const int keys = max(khi - klo + 1, 0);       // the keys this workgroup sweeps
#elif QATTN_SKV_WINDOW
    // [klo, khi]: the keys of the split that the tile's valid rows attend
    const int klo = max(k_begin, wn.left < 0 ? 0 : clampl((long)smin + win_lo, 0, L));
    const int khi = min(k_end - 1, clampl((long)smax + win_hi, -1, L - 1));
    const int keys = max(khi - klo + 1, 0);       // the keys this workgroup sweeps
#else
    const int delta = L - SKV_SQ;   // causal: position p attends the keys j <= p + delta
    const int khi = a.causal ? min(k_end - 1, smax + delta) : k_end - 1;
    const int keys = max(khi - k_begin + 1, 0);   // the keys this workgroup sweeps
#endif
    if (sel == kFpvSelMany && keys < a.two_term_keys) return;
    if (sel == kFpvSelFew && keys >= a.two_term_keys) return;

    const int r = r_first + wave * kQPerWave + ql;   // packed row
    const bool rvalid = r < SKV_ROWS;
    const int g = min(r / SKV_SQ, a.G - 1);          // (padding rows: the last head's scale)
#if QATTN_SKV_VARQ
    // q8 is the packed pre-pass's: sequence i's [Hq, Sq_i, D] slab at row Hq start_i, the kv head's packed rows consecutive in it; the
    // outputs are packed by token.  (A padding row's token may lie outside the sequence: every use is under rvalid.)
    const int tok = q_start + (r - g * Sq_i), head = hkv * a.G + g;
    const long qrow0 = (long)vq.Hq * q_start + (long)hkv * rows_i, qrow = qrow0 + r;
    const long orow = (long)tok * vq.Hq + head, lrow = (long)head * vq.total_q + tok;
#else
    const long grow = (long)kvh * a.rows + r;        // row of the dense [B Hq Sq] index space
#endif
    if (keys == 0) {   // no key for any row of the tile in this split (L = 0, a split past the last block, a split above the causal edge)
        if (a.ns == 1) {
#if QATTN_SKV_SINK
            // the sink alone: zero rows with LSE = sink (-inf: the window kernel's empty row); +inf and NaN make the rows NaN
            const float snk = sn.sink[SKV_HEAD];
            const float sink1 = snk < INFINITY ? snk : NAN;
            v16f z[MB];
#pragma unroll
            for (int m = 0; m < MB; m++)
#pragma unroll
                for (int e = 0; e < 16; e++) z[m][e] = 0.0f;
            store_o_rows<MB>(a.out, a.out_fmt, z, sink1 != sink1 ? sink1 : 0.0f, (rvalid ? SKV_OROW : 0L) * (2L * D), hh, rvalid);
            if (a.lse && hh == 0 && rvalid) a.lse[SKV_LROW] = sink1;
            if (a.path && hh == 0 && rvalid) a.path[SKV_LROW] = (unsigned char)QATTN_PATH_ONE_TERM;
#else
            fpv_store_empty<D>(a.out, a.out_fmt, (rvalid ? SKV_OROW : 0L) * (2L * D), a.lse, SKV_LROW, a.path, SKV_LROW, hh, rvalid);
#endif
        } else {
            const long prow = (long)s * a.part_rows + (rvalid ? SKV_OROW : 0L), plrow = (long)s * a.part_rows + (rvalid ? SKV_LROW : 0L);
            v16f z[MB];
#pragma unroll
            for (int m = 0; m < MB; m++)
#pragma unroll
                for (int e = 0; e < 16; e++) z[m][e] = 0.0f;
            store_o_rows_f32<MB>(a.po + prow * D, z, 0.0f, hh, rvalid);
            if (hh == 0 && rvalid) a.plse[plrow] = -INFINITY;
            if (a.ppath && hh == 0 && rvalid) a.ppath[plrow] = (unsigned char)QATTN_PATH_ONE_TERM;
        }
        return;
    }
#if QATTN_SKV_WINDOW
    const int c_first = klo >> 6;                   // chunks c_first .. khi / 64 <= (L - 1) / 64 < nchunks: no other chunk is fetched
#else
    const int c_first = k_begin >> 6;               // chunks c_first .. khi / 64 <= (L - 1) / 64 < nchunks
#endif
    const int n_wg = (khi >> 6) - c_first + 1;

#if QATTN_SKV_PAGED
    // The ring's base is the pool itself; a step's chunk is (page Hkv + hkv) pc + its chunk within the page.  (p_idx, p_ch) count pages and
    // chunks-in-page along the sweep -- one division here, none in the loop -- and always stand at the chunk whose DMA is issued NEXT;
    // e_next is the RAW table entry of that chunk's page, loaded when the sweep enters the page: a step before the DMA that needs it.
    // The chunks c_first .. c_first + n_wg - 1 lie below ceil(L / 64), so their entries lie below ceil(L / page_size) <= max_pages: the
    // only ones read.  skv_phys clamps an entry where it forms the address.
    const int phk = kvh % a.Hkv;
    const int* prow = pg.table + (long)(kvh / a.Hkv) * pg.stride;
    int p_idx = c_first / pg.pc, p_ch = c_first % pg.pc;
    FpvRing<D> ring(smem, wave, lane, a.k8 + (wave << 10), a.v8 + (wave << 10));
    int e_next = prow[p_idx];
    ring.dma_chunk(skv_phys(pg, e_next, a.Hkv, phk, p_ch));
    if (++p_ch == pg.pc) {
        p_ch = 0;
        p_idx++;
        if (n_wg > 1) e_next = prow[p_idx];
    }
#else
    const long img = (long)kvh * a.nchunks * CH + (wave << 10);
    FpvRing<D> ring(smem, wave, lane, a.k8 + img, a.v8 + img);
    ring.dma_chunk(c_first);
#endif
    sw.park_q(a.q8 + (rvalid ? SKV_QROW : SKV_QROW0) * D + hh * 32, rvalid);
    constexpr float kNoKeyYet = -1.0e20f;   // (attn_vfp8_window_kernel's header comment)
#if QATTN_SKV_SOFTCAP
    // the sweep sees t = tanh(x / softcap): its scores -> log2 units factor is softcap log2e, and this row's raw score -> exponent of the
    // tanh factor is kin2 (the row's own head's scale_q: the tile may hold several heads)
    sw.init_state(sc.c, kNoKeyYet);
    const float kin2 = sc.kin2 * a.sq[(long)kvh * a.G + g] * a.sk[kvh];
#else
    sw.init_state(a.sm_log2e * a.sq[(long)kvh * a.G + g] * a.sk[kvh], kNoKeyYet);
#endif
    const int one = fpv_ones_word(lane);
#if QATTN_SKV_WINDOW
    // the first and the last key this lane's row attends (a padding row: position >= Sq, masked as attn_vfp8_window_kernel masks it), and
    // where a chunk crosses an edge of some valid row: its end above `edge`, its start below `edge_lo`
    const long pos = (long)r - (long)g * SKV_SQ;
#if QATTN_SKV_TREE
    // the word of this lane's token, as in the tree text below, and the row's depth in the position's place at the window's lower edge
    const bool tree_l = SKV_SQ <= 64 && rvalid;
    const unsigned long long tword = tree_l ? tr.mask[tok] : ~0ull;
    const int tree_lo = SKV_SQ <= 64 ? (int)max(delta, 0L) : INT_MAX;
    const long dep = tree_l ? (long)__builtin_popcountll(tword & ((1ull << (int)pos) - 1ull)) : pos;
    const int lo_l = wn.left < 0 ? 0 : clampl(dep + win_lo, 0, L);
    const int hi_l = clampl(pos + win_hi, -1, L - 1);
    const int edge = clampl((long)smin + win_hi, -1, L);
    const int edge_lo = wn.left < 0 ? 0 : clampl((long)dmax + win_lo, 0, L);
#else
    const int lo_l = wn.left < 0 ? 0 : clampl(pos + win_lo, 0, L);
    const int hi_l = clampl(pos + win_hi, -1, L - 1);
    const int edge = clampl((long)smin + win_hi, -1, L);
    const int edge_lo = wn.left < 0 ? 0 : clampl((long)smax + win_lo, 0, L);
#endif
    // The keys below lo_i that share its chunk: no row attends them, so their P is exactly 0 -- and 0 x NaN is NaN in the matrix pipe.
    // The workgroup whose first chunk holds lo_i zeroes their V bytes once the stage has landed, before anyone reads it (the mirror of
    // skv_zero_v_tail; K needs nothing).
    if ((c_first << 6) < lo_i) {
        sw.wait_stage();
        skv_zero_v_head<D>(smem + CH, lo_i - (c_first << 6));
    }
#else
    // the last key this lane's row attends, and the first chunk end that crosses the causal edge of some valid row
    const int hi_l = (a.causal && rvalid) ? min(L - 1, r - g * SKV_SQ + delta) : L - 1;
    const int edge = a.causal ? smin + delta : INT_MAX;
#if QATTN_SKV_TREE
    // the word of this lane's token -- every head of the token reads the same one; a padding row and a sequence with more than 64 queries
    // (plain causal) read none -- and the first draft key: a chunk that ends at or above it takes the token branch
    const bool tree_l = SKV_SQ <= 64 && rvalid;
    const unsigned long long tword = tree_l ? tr.mask[tok] : ~0ull;
    const int tree_lo = SKV_SQ <= 64 ? max(delta, 0) : INT_MAX;
#endif
#endif

    for (int t = 0; t < n_wg; t++) {   // step t sweeps chunk c_first + t
        const int k0 = (c_first + t) * 64;
        if (__builtin_expect(k0 + 64 > L, 0)) {   // the chunk that holds key L: its stage is waited for here, ahead of the step's own (then idle) wait
            sw.wait_stage();
            skv_zero_v_tail<D>(smem + (t & 1) * (2 * CH) + CH, L - k0);
        }
        v8i qf[KS];
        sw.read_q(qf);
        sw.wait_stage();
#if QATTN_SKV_PAGED
        if (t + 1 < n_wg) {
            ring.dma_chunk(skv_phys(pg, e_next, a.Hkv, phk, p_ch));
            if (++p_ch == pg.pc) {   // the chunk after this one opens a page: its entry is in flight during this step's products
                p_ch = 0;
                p_idx++;
                if (t + 2 < n_wg) e_next = prow[p_idx];
            }
        }
#else
        if (t + 1 < n_wg) ring.dma_chunk(c_first + t + 1);
#endif
        v16f s0, s1;
        v8i vf0, vf1;
        sw.qk(t, qf, s0, s1, vf0, vf1);
#if QATTN_SKV_SOFTCAP
        // ---- the cap, on all 32 scores of every chunk and BEFORE the mask: s -> tanh(s kin) = 1 - 2 / (1 + 2^(s kin2)).  Eight scores at a
        // time: the empty asm hands the eight results and kq on, so that the next eight start after these -- eight independent chains keep
        // the transcendental pipe full, and all 32 in flight at once cost the D = 256 kernels more registers than they have.
        float kq = kin2;
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            float x[8];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                x[u] = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s0[e + u] * kq)), 1.0f);
                x[4 + u] = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s1[e + u] * kq)), 1.0f);
            }
            asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "+v"(kq));
#pragma unroll
            for (int u = 0; u < 4; u++) {
                s0[e + u] = x[u];
                s1[e + u] = x[4 + u];
            }
        }
#endif
#if QATTN_SKV_WINDOW && QATTN_SKV_TREE
        // ---- the ragged tail at L, the window's two edges and the draft tree by token, under a workgroup-uniform condition
        if (__builtin_expect(k0 + 64 > L || k0 + 63 > edge || k0 < edge_lo || k0 + 63 >= tree_lo, 0)) {
            // bit i of aw: key k0 + i passes the tree, as in the tree text below.  (With a word: -L <= k0 - delta < 64 + Sq_i, an int.)
            const int sh = (int)((long)k0 - delta);
            unsigned long long aw = ~0ull;
            if (tree_l) aw = sh >= 64 ? 0ull : sh >= 0 ? tword >> sh : sh > -64 ? (tword << -sh) | ((1ull << -sh) - 1ull) : ~0ull;
            aw >>= 4 * hh;
            const int base = k0 + 4 * hh;
#pragma unroll
            for (int e = 0; e < 32; e++) {
                const int kb = 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);   // (kb + 4 hh <= 63)
                const int key = base + kb;
                v16f& sx = (e >> 4) ? s1 : s0;
                sx[e & 15] = (key < lo_l || key > hi_l || !((aw >> kb) & 1ull)) ? -INFINITY : sx[e & 15];
            }
        }
#elif QATTN_SKV_WINDOW
        // ---- the ragged tail at L and the window's two edges by token, under a workgroup-uniform condition
        if (__builtin_expect(k0 + 64 > L || k0 + 63 > edge || k0 < edge_lo, 0)) {
            const int base = k0 + 4 * hh;
#pragma unroll
            for (int e = 0; e < 32; e++) {
                const int key = base + 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);
                v16f& sx = (e >> 4) ? s1 : s0;
                sx[e & 15] = (key < lo_l || key > hi_l) ? -INFINITY : sx[e & 15];
            }
        }
#elif QATTN_SKV_TREE
        // ---- the ragged tail at L, the causal edge and the draft tree by token, under a workgroup-uniform condition
        if (__builtin_expect(k0 + 64 > L || k0 + 63 > edge || k0 + 63 >= tree_lo, 0)) {
            // bit i of aw: key k0 + i passes the tree.  Key j is bit j - delta of the word; the keys below delta are committed ones and
            // pass; a key at or above delta + 64 lies above every causal edge of a sequence with a tree.  (k0 - delta < Sq_i: an int.)
            const int sh = k0 - delta;
            unsigned long long aw = ~0ull;
            if (tree_l) aw = sh >= 64 ? 0ull : sh >= 0 ? tword >> sh : sh > -64 ? (tword << -sh) | ((1ull << -sh) - 1ull) : ~0ull;
            aw >>= 4 * hh;
            const int base = k0 + 4 * hh;
#pragma unroll
            for (int e = 0; e < 32; e++) {
                const int kb = 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);   // (kb + 4 hh <= 63)
                const int key = base + kb;
                v16f& sx = (e >> 4) ? s1 : s0;
                sx[e & 15] = (key > hi_l || !((aw >> kb) & 1ull)) ? -INFINITY : sx[e & 15];
            }
        }
#else
        // ---- the ragged tail at L and the causal edge by token, under a workgroup-uniform condition
        if (__builtin_expect(k0 + 64 > L || k0 + 63 > edge, 0)) {
            const int base = k0 + 4 * hh;
#pragma unroll
            for (int e = 0; e < 32; e++) {
                const int key = base + 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);
                v16f& sx = (e >> 4) ? s1 : s0;
                sx[e & 15] = key > hi_l ? -INFINITY : sx[e & 15];
            }
        }
#endif
        sw.softmax_pv(s0, s1, vf0, vf1, two, [&] { return fpv_spread_ones(one); });
    }

    // ---- epilogue (V's one scale per kv head is applied here)
    const float l_tot = sw.row_sum();
    const bool has_key = l_tot > 0.0f;   // (a row without a key inside a workgroup that sweeps: every P was 0 -- a zero row, LSE -inf)
    const float inv = has_key ? a.sv[kvh] / l_tot : 0.0f;
    const float lse_row = has_key ? 0.6931471805599453f * (sw.m_run * sw.c - kPShift) + __logf(l_tot) : -INFINITY;
    const unsigned char code = (unsigned char)((!BYTE && two) ? QATTN_PATH_TWO_TERM : QATTN_PATH_ONE_TERM);
    if (a.ns == 1) {
#if QATTN_SKV_SINK
        // The sink joins the row's sum under the sweep's own shift: P' = 2^(x c - base), base = m_run c - kPShift, so the sink's term is
        // e = 2^(sink log2e - base).  (Loaded here, after the loop; a padding row reads the sink of head G - 1 and stores nothing.)
        const float snk = sn.sink[SKV_HEAD];
        const float sink1 = snk < INFINITY ? snk : NAN;   // +inf, NaN: the head's rows are NaN
        float inv_s, lse_s;
        if (has_key) {
            const float d = sink1 * 1.4426950408889634f - (sw.m_run * sw.c - kPShift);
            if (d > 64.0f) {   // a sink far above every score: sum under the SINK's shift instead, so that e cannot overflow
                const float r = __builtin_amdgcn_exp2f(-d);
                const float l_s = l_tot * r + 1.0f;
                inv_s = a.sv[kvh] * r / l_s;
                lse_s = sink1 + __logf(l_s);
            } else {           // (sink = -inf: e = 0, and l_tot + 0.0f is l_tot -- the bits of the kernel without a sink)
                const float l_s = l_tot + __builtin_amdgcn_exp2f(d);
                inv_s = a.sv[kvh] / l_s;
                lse_s = 0.6931471805599453f * (sw.m_run * sw.c - kPShift) + __logf(l_s);
            }
        } else {               // no key for this row (m_run may still stand at its start value: it is not read): the sink alone
            inv_s = sink1 != sink1 ? sink1 : 0.0f;
            lse_s = sink1;
        }
        store_o_rows<MB>(a.out, a.out_fmt, sw.o, inv_s, (rvalid ? SKV_OROW : 0L) * (2L * D), hh, rvalid);
        if (!BYTE && a.lse && hh == 0 && rvalid) a.lse[SKV_LROW] = lse_s;
        if (a.path && hh == 0 && rvalid) a.path[SKV_LROW] = code;
#else
        store_o_rows<MB>(a.out, a.out_fmt, sw.o, inv, (rvalid ? SKV_OROW : 0L) * (2L * D), hh, rvalid);
        if (!BYTE && a.lse && hh == 0 && rvalid) a.lse[SKV_LROW] = lse_row;
        if (a.path && hh == 0 && rvalid) a.path[SKV_LROW] = code;
#endif
    } else {
        const long prow = (long)s * a.part_rows + (rvalid ? SKV_OROW : 0L), plrow = (long)s * a.part_rows + (rvalid ? SKV_LROW : 0L);
        store_o_rows_f32<MB>(a.po + prow * D, sw.o, inv, hh, rvalid);
        if (!BYTE && hh == 0 && rvalid) a.plse[plrow] = lse_row;
        if (a.ppath && hh == 0 && rvalid) a.ppath[plrow] = code;
    }
#undef SKV_SQ
#undef SKV_ROWS
#undef SKV_QROW
#undef SKV_QROW0
#undef SKV_OROW
#undef SKV_LROW
#undef SKV_HEAD
