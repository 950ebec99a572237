// qattn_kvcache_append_body.h -- the BODY of the append kernel, included inside the two kernel definitions of qattn_kvcache_append.h (no
// include guard: it is text, not declarations).  QATTN_KVA_PAGED selects where the workgroup's chunk is stored: 0, the contiguous image --
// statement for statement the kernel qattn_kvcache_append.hip held before the paged entry existed, so that its device code stays what it
// was; 1, the pool through the block table `pg` (include/qattn_paged.h).  Shared as text, not as an inlined function, for the reason
// qattn_splitkv_body.h gives.
// QATTN_KVA_VARQ (with QATTN_KVA_PAGED; include/qattn_paged_varlen_append.h) selects where the workgroup's TOKENS live: 0, the padded
// [B, Hkv, T, D] tensors, new_lens[b] of sequence b's T rows used; 1, packed tensors [total, Hkv, D] cut by cu_seqlens (`vq`, KvVarq): the
// workgroup finds its (sequence, chunk) by a binary search on the chunk-slot bases 2 i + start_i / 64 -- the search QATTN_SKV_VARQ runs on
// its tile slots (qattn_splitkv_body.h) -- and the sequence's count end_i - start_i stands where the padded kernels clamp new_lens[b].
// With the switch off the text the compiler sees is what it was.
// QATTN_KVA_ROPE (with QATTN_KVA_PAGED and QATTN_KVA_VARQ; include/qattn_paged_varlen_rope.h) rotates K between the load and the quantiser:
// the K half (blockIdx.y = 0) holds the work units of qattn_rope_dev.h -- the 16-byte pieces dvh and dvh + D/16 of one row in one thread,
// ITERS / 2 units in the same ITERS registers -- so that no value crosses lanes; a unit of chunk row r in [lo, hi) is key key0 + r of its
// sequence and rotates with table row min(key0 + r, T - 1) (`rp`, KvRope; template flag IL = interleaved pairs).  The rotated vector is
// rounded to the input dtype (rope_unit) before has_nonfinite16 and quant8 see it, and lands at the LDS offsets the plain mapping uses;
// everything behind the barrier, and the V half, is the shared text.  With the switch off the text the compiler sees is what it was.
// QATTN_KVA_POS (with QATTN_KVA_ROPE; include/qattn_paged_varlen_rope_pos.h; not defined by the other compilations: off) takes the table
// row of a key from the caller's 64-bit positions tensor (`ps`, KvPos), indexed by the key's TOKEN, instead of from the key's index:
// the one line that forms `pos`.  Where the key is stored does not change.
// In scope: template parameters D, IN_FMT, OUT_FMT (rope: IL); arguments a (KvAppendArgs), -- paged -- pg (KvPages), -- packed -- vq
// (KvVarq), -- rope -- rp (KvRope) and -- positions -- ps (KvPos).
    constexpr int VPR = D / 8;             // 16-byte input vectors per row
    constexpr int ITERS = 64 * VPR / 256;  // vectors per thread
    constexpr int KPAD = 64 * D + (64 * D / 512) * 16;  // KFRAG image + 16 B per 512 B     (the staging images of quant_multi_kernel)
    constexpr int VSTRIDE = D + 4;                      // VFRAG staging: fp8 row-major
    constexpr int LDS_BYTES = KPAD > 64 * VSTRIDE ? KPAD : 64 * VSTRIDE;
    __shared__ __attribute__((aligned(16))) unsigned char img[LDS_BYTES];
    const int tid = threadIdx.x, z = blockIdx.y;
#if QATTN_KVA_VARQ
    // blockIdx.x = h NS + j: chunk slot j of kv head h.  Slot j belongs to the largest sequence i with base_i = 2 i + start_i / 64 <= j, as
    // the chunk j - base_i counted from the one that holds key p_i; base_{i+1} - base_i >= n_i / 64 + 2, the most chunks n_i keys touch
    const int h = (int)(blockIdx.x / (unsigned)vq.NS), jt = (int)(blockIdx.x % (unsigned)vq.NS);
    int b = 0, b_hi = vq.B - 1;
    while (b < b_hi) {   // (workgroup-uniform)
        const int mid = (b + b_hi + 1) >> 1;
        const int sm = kv_clampi(__builtin_amdgcn_readfirstlane(vq.cu[mid]), 0, vq.total);
        if (2 * mid + sm / 64 <= jt) b = mid;
        else b_hi = mid - 1;
    }
    const int start = kv_clampi(__builtin_amdgcn_readfirstlane(vq.cu[b]), 0, vq.total);
    const int n = kv_clampi(__builtin_amdgcn_readfirstlane(vq.cu[b + 1]), start, vq.total) - start;
    const int ci = jt - (2 * b + start / 64);
    if (ci < 0 || ci > n / 64 + 1) return;   // a slot that is no chunk of its sequence: before any other memory is touched
    const int g = b * a.Hkv + h;
    int p = a.seqlens[b];
    p = p < 0 ? 0 : p > a.capacity ? a.capacity : p;
    const int end = a.capacity - p >= n ? p + n : a.capacity;   // (kv_append_range on the sequence's own count)
#else
    const int g = (int)(blockIdx.x / (unsigned)a.nchunk), ci = (int)(blockIdx.x % (unsigned)a.nchunk);
    const int b = g / a.Hkv, h = g % a.Hkv;
    int p, end;
    kv_append_range(a.seqlens, a.new_lens, b, a.T, a.capacity, p, end);
#endif
    const long key0 = 64L * (p / 64 + ci);   // first key of this workgroup's chunk
    if (p >= end || key0 >= end) return;     // (workgroup-uniform: nothing is appended -- new_lens 0, a full cache -- or nothing of this chunk)
    // the chunk's keys [lo, hi) are the tokens [key0 + lo - p, key0 + hi - p) of the call
    const int lo = p > key0 ? (int)(p - key0) : 0, hi = end - key0 < 64 ? (int)(end - key0) : 64;
    const float scale = a.scale[z][g];
    const float rinv = 1.0f / scale;
#if QATTN_KVA_VARQ
    // key p + t is token start + t < start + n <= total: the rows [lo, hi) of the chunk are rows of the sequence's own tokens
    const uint4* xg = a.x[z] + (long)h * a.sh[z] + ((long)start + key0 - p) * a.st[z];   // row of chunk key 0 (not touched below lo)
#else
    const uint4* xg = a.x[z] + (long)b * a.sb[z] + (long)h * a.sh[z] + (key0 - p) * a.st[z];   // row of chunk key 0 (not touched below lo)
#endif
    const long st = a.st[z];
    uint4 held[ITERS];
#if QATTN_KVA_ROPE
    if (z == 0) {   // (workgroup-uniform)
        constexpr int HV = D / 16;   // units per row; 64 HV / 256 = ITERS / 2 units per thread
        const float4* cg = reinterpret_cast<const float4*>(rp.cs);
        const float4* sg = reinterpret_cast<const float4*>(rp.sn);
        const long tr4 = rp.tr >> 2;
        float4 c[ITERS / 2][2], s[ITERS / 2][2];
#pragma unroll
        for (int u = 0; u < ITERS / 2; u++) {
            const int unit = u * 256 + tid;
            const int r = unit / HV, dvh = unit % HV;
            held[2 * u] = held[2 * u + 1] = make_uint4(0, 0, 0, 0);
            c[u][0] = c[u][1] = s[u][0] = s[u][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r >= lo && r < hi) {   // (rows outside: zero vectors, no table row read)
                const uint4* px = xg + (long)r * st + dvh;
                held[2 * u] = load_nt(px);
                held[2 * u + 1] = load_nt(px + HV);
#if QATTN_KVA_POS
                // key key0 + r is token start + key0 + r - p < start + n <= total of the call: its position is the caller's, clamped in 64
                // bits so that the row stays inside the tables whatever the tensor holds
                const long long want = ps.pos[(long)start + key0 + r - p];
                const int pos = want < 0 ? 0 : want < rp.T ? (int)want : rp.T - 1;
#else
                // key0 + r < end <= capacity: an int; the clamp keeps the row inside the tables whatever seqlens holds
                const int pos = (int)key0 + r < rp.T ? (int)key0 + r : rp.T - 1;
#endif
                const int t0 = IL ? dvh : 2 * dvh, t1 = IL ? dvh + HV : 2 * dvh + 1;
                c[u][0] = cg[pos * tr4 + t0]; c[u][1] = cg[pos * tr4 + t1];
                s[u][0] = sg[pos * tr4 + t0]; s[u][1] = sg[pos * tr4 + t1];
            }
        }
#pragma unroll
        for (int u = 0; u < ITERS / 2; u++) {
            const int unit = u * 256 + tid;
            const int r = unit / HV, dvh = unit % HV;
            if (r >= lo && r < hi) rope_unit<IN_FMT, IL>(held[2 * u], held[2 * u + 1], c[u], s[u]);
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const uint4& y = held[2 * u + half];
                const int2 lohi = quant8<IN_FMT, OUT_FMT>(y, scale, rinv, has_nonfinite16<IN_FMT>(y));   // (on the ROTATED vector)
                const int o = kfrag_offset<D>(r, (dvh + half * HV) * 8);
                *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
            }
        }
    } else {
#endif
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid;
        const int r = vec / VPR;
        held[it] = make_uint4(0, 0, 0, 0);
        if (r >= lo && r < hi) held[it] = load_nt(xg + (long)r * st + vec % VPR);
    }
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid;
        const int r = vec / VPR, d0 = (vec % VPR) * 8;
        const int2 lohi = quant8<IN_FMT, OUT_FMT>(held[it], scale, rinv, has_nonfinite16<IN_FMT>(held[it]));   // NaN stays NaN, +-inf clamps to +-qmax
        if (z == 0) {
            const int o = kfrag_offset<D>(r, d0);
            *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
        } else {
            *reinterpret_cast<int*>(img + r * VSTRIDE + d0) = lohi.x;
            *reinterpret_cast<int*>(img + r * VSTRIDE + d0 + 4) = lohi.y;
        }
    }
#if QATTN_KVA_ROPE
    }
#endif
    __syncthreads();
#if QATTN_KVA_PAGED
    // key0 < end <= capacity = max_pages page_size: the entry read is one of the pages that cover [p, end); its clamp keeps the chunk inside
    // the pool whatever the table holds
    const int cs = (int)(key0 >> 6);
    int page = pg.table[(long)b * pg.stride + cs / pg.pc];
    page = page < 0 ? 0 : page > pg.num_pages - 1 ? pg.num_pages - 1 : page;
    unsigned char* og = a.img[z] + (((long)page * a.Hkv + h) * pg.pc + cs % pg.pc) * (64L * D);   // the chunk in the pool
#else
    const long Sp = ((long)a.capacity + 63) / 64 * 64;
    unsigned char* og = a.img[z] + ((long)g * Sp + key0) * D;   // the chunk in the image
#endif
    const bool whole = lo == 0 && hi == 64;
    if (z == 0) {
        // piece i of a KFRAG chunk = [t:2][s:D/64][hh:2][half:2][key:32] holds 16 channels of ONE key, 32 t + key
        for (int i = tid; i < 64 * D / 16; i += 256) {
            const int r = 32 * (i / (2 * D)) + (i & 31);
            if (whole || (r >= lo && r < hi)) reinterpret_cast<uint4*>(og)[i] = *reinterpret_cast<const uint4*>(img + i * 16 + ((i >> 5) << 4));
        }
    } else if (whole) {
        vfrag_copy_out<D, VSTRIDE>(img, og, tid);
    } else {
        // word wd of a VFRAG chunk = [m:D/32][hh:2][half:2][d:32][w:4] holds channel 32 m + d of the 4 keys 32 half + 8 w + 4 hh + (0..3):
        // a word store where all four are appended, byte stores of the appended ones otherwise -- the others' bytes are neither read nor written
        for (int wd = tid; wd < 64 * D / 4; wd += 256) {
            const int w = wd & 3, dl = (wd >> 2) & 31, half = (wd >> 7) & 1, hh = (wd >> 8) & 1, m = wd >> 9;
            const int kb = 32 * half + 8 * w + 4 * hh;
            if (kb + 4 <= lo || kb >= hi) continue;
            const unsigned char* src = img + kb * VSTRIDE + 32 * m + dl;
            const unsigned b0 = src[0], b1 = src[VSTRIDE], b2 = src[2 * VSTRIDE], b3 = src[3 * VSTRIDE];
            if (kb >= lo && kb + 4 <= hi) {
                *reinterpret_cast<unsigned*>(og + 4 * wd) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
            } else {
                const unsigned bytes[4] = {b0, b1, b2, b3};
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (kb + i >= lo && kb + i < hi) og[4 * wd + i] = (unsigned char)bytes[i];
            }
        }
    }
