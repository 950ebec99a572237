// qattn_merge_body.h -- the BODY of the state-merge kernel, included inside the kernel definitions of qattn_merge.hip and
// qattn_merge_sink.hip (no include guard: it is text, not declarations -- the way qattn_splitkv_body.h is shared).
// QATTN_MERGE_SINK: 0, the kernel of include/qattn_merge.h, token for token what qattn_merge.hip held; 1, a learned sink per head `sink[h]`
// (include/qattn_sinks.h) is one more state of the row with lse = sink[h] and no O row: it joins the maximum after the partials, is
// summed into den after them, and takes part in the "all partials empty" decision.  sink[h] = -inf adds exp(-inf) = 0.0f: the bits of the
// kernel without it.
// In scope: template parameters D, N; argument p (MergeParams) and -- sink -- sink.
    constexpr int kLanes = D / 8;          // lanes of one row
    constexpr int kRows = 256 / kLanes;    // rows of one workgroup
    const int piece = (int)threadIdx.x % kLanes;
    const long long s = (long long)blockIdx.x * kRows + (int)threadIdx.x / kLanes;
    if (s >= p.S) return;
    const long long b = blockIdx.z, h = blockIdx.y;

    // every load of the row first: N floats and N (fp32: 2 N) 16-byte pieces, none depending on another
    float l[N];
    uint4 ra[N], rb[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        l[i] = p.lse[i][b * p.ls[i][0] + h * p.ls[i][1] + s * p.ls[i][2]];
        const long long e = b * p.os[i][0] + h * p.os[i][1] + s * p.os[i][2] + piece * 8;
        if (p.fmt[i] == QATTN_FMT_FP32) {
            const uint4* src = reinterpret_cast<const uint4*>(static_cast<const float*>(p.o[i]) + e);
            ra[i] = src[0];
            rb[i] = src[1];
        } else {
            ra[i] = *reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(p.o[i]) + e);
            rb[i] = ra[i];
        }
    }
#if QATTN_MERGE_SINK
    const float snk = sink[h];
#endif

    // m = max_i lse_i; a NaN stays (fmaxf would drop it)
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < N; i++) m = (l[i] > m || l[i] != l[i]) ? l[i] : m;
#if QATTN_MERGE_SINK
    m = (snk > m || snk != snk) ? snk : m;
#endif

    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float lse_row = -INFINITY;
    if (m != -INFINITY) {   // (all partials empty: the zero row and -inf above)
        float den = 0.f;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const float w = expf(l[i] - m);   // +inf - +inf, NaN: NaN, and it spreads over the row
            den += w;
            float x[8];
            if (p.fmt[i] == QATTN_FMT_FP32) {
                const float t[8] = {__uint_as_float(ra[i].x), __uint_as_float(ra[i].y), __uint_as_float(ra[i].z), __uint_as_float(ra[i].w),
                                    __uint_as_float(rb[i].x), __uint_as_float(rb[i].y), __uint_as_float(rb[i].z), __uint_as_float(rb[i].w)};
#pragma unroll
                for (int j = 0; j < 8; j++) x[j] = t[j];
            } else if (p.fmt[i] == QATTN_FMT_BF16) {
                merge_unpack16<QATTN_FMT_BF16>(ra[i], x);
            } else {
                merge_unpack16<QATTN_FMT_FP16>(ra[i], x);
            }
            // a partial of weight zero (lse_i = -inf, or too far below m) contributes nothing WHATEVER its row holds: 0 * NaN would be NaN
            const bool live = w != 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] += w * (live ? x[j] : 0.f);
        }
#if QATTN_MERGE_SINK
        // the sink's weight, last in the sum.  A NaN sink has made every w NaN above; a +inf sink is m, every w is 0 and this term NaN
        // (+inf - +inf): 0 x the NaN reciprocal below makes the row NaN either way
        den += expf(snk - m);
#endif
        const float inv = 1.0f / den;
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] *= inv;
        lse_row = m + logf(den);
    }

    const long long eo = b * p.outs[0] + h * p.outs[1] + s * p.outs[2] + piece * 8;
    if (p.out_fmt == QATTN_FMT_FP32) {
        float4* dst = reinterpret_cast<float4*>(static_cast<float*>(p.out) + eo);
        dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
        uint4 r;
        if (p.out_fmt == QATTN_FMT_BF16) {
            r = make_uint4(merge_pack16<QATTN_FMT_BF16>(acc[0], acc[1]), merge_pack16<QATTN_FMT_BF16>(acc[2], acc[3]),
                           merge_pack16<QATTN_FMT_BF16>(acc[4], acc[5]), merge_pack16<QATTN_FMT_BF16>(acc[6], acc[7]));
        } else {
            r = make_uint4(merge_pack16<QATTN_FMT_FP16>(acc[0], acc[1]), merge_pack16<QATTN_FMT_FP16>(acc[2], acc[3]),
                           merge_pack16<QATTN_FMT_FP16>(acc[4], acc[5]), merge_pack16<QATTN_FMT_FP16>(acc[6], acc[7]));
        }
        *reinterpret_cast<uint4*>(static_cast<unsigned short*>(p.out) + eo) = r;
    }
    // in place (lse_out = lse[0]): the lanes of a row sit in one wave and have all read lse[0] of the row above
    if (p.lse_out != nullptr && piece == 0) p.lse_out[b * p.louts[0] + h * p.louts[1] + s * p.louts[2]] = lse_row;
