/*
 * qattn_buffers.h -- the BUFFER CONTRACT of every entry of qattn.h, qattn_strided.h, qattn_smooth.h, qattn_varlen.h, qattn_window.h and
 * qattn_block_sparse.h, and of qattn_rope.h, qattn_splitkv.h, qattn_kvcache.h, qattn_paged.h, qattn_paged_varlen.h and qattn_splitkv_window.h
 * (documentation only: no declaration).  Held by
 * tests/test_gpu_buffer_contract.py (qattn_rope.h: tests/test_gpu_rope_buffer_contract.py; qattn_splitkv.h:
 * tests/test_gpu_splitkv_buffer_contract.py; qattn_kvcache.h: tests/test_gpu_kvcache_buffer_contract.py; qattn_paged.h:
 * tests/test_gpu_paged_buffer_contract.py) on guarded buffers of exactly these sizes at exactly these alignments.
 *
 *   sizes      a buffer of qattn_*_tensor_bytes / qattn_lse_row_stride / *_workspace_bytes bytes (or of the stated shape) suffices; no entry
 *              reads or writes a byte before a buffer's start or past its end, ragged last tiles included, and no result depends on bytes
 *              outside the inputs (the pads between the rows / heads of a strided view included) or on what a workspace or an output held.
 *   alignment  16 bytes (the kernels' widest access: dwordx4 loads / stores, LDS-DMA rows): q / k / v / out and their 8-bit images (q8, k8, v8,
 *              x8, fragment images), every workspace, k_mean.  4 bytes: fp32 scale_*, amax_*, ssq_*, lse (read and written one float at a
 *              time, or as float4 runs at whatever offset a head's rows start: token-wise scale_k) and the int32 tables.  1 byte: row_path,
 *              block_mask.  More alignment is never assumed.
 *   written    every element of out, lse (REFERENCE layout: the Sq floats of each row, not the pad up to the row stride), row_path, scale_q,
 *              scale_k, k_mean and of a quantiser's / packer's own outputs (fragment images: the zero padding up to 64 keys included); of a
 *              strided `out` only the D elements of each row -- the pads between rows and heads keep what they held.  The fused entries
 *              (qattn.h: qattn_fp8_quant_attention_forward) also write ALL of k8, of q8 where the PATH TABLE says q_quant = prepass (the
 *              pre-pass's row-major image = qattn_quant_qkv_fp8's) and of v8 / scale_v where v_format = head (per-head VFRAG image and scale).
 *   scratch    not for a caller to read: q8 of the fused entries where q_quant = kernel (untouched); their v8 / scale_v where v_format =
 *              block (bytes under per-chunk scales kept in the workspace; scale_v = 1); the packed entries' k8 between the sequences'
 *              images (qattn_varlen.h: the images of the used keys do not tile the buffer).
 *
 * qattn_fp8_quant_attention_varlen_forward_fp8pv (qattn_varlen.h), beyond what the packed entries above state for q8 / k8 / scale_q / scale_k:
 *   v8         qattn_varlen_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, total_k, D) bytes (k8's size), 16-byte aligned.  Written: sequence i's VFRAG image,
 *              Hkv ceil(L_k/64) 64 D bytes from byte Hkv D (cu_k[i] + 64 i) (L_k its used keys; the zero padding up to 64 keys included).
 *              Scratch between the images: as k8's, the images of the used keys do not tile the buffer.
 *   scale_v    fp32 [B, Hkv], 4-byte aligned; every element written (a sequence without a used key: the quantiser's eps).
 *   row_path   uint8 [Hq, total_q], 1-byte aligned; written: the columns cu_q[i] .. cu_q[i+1]-1 of every sequence, the others keep what they held.
 *   k_mean     fp32 [B, Hkv, D], 16-byte aligned; every element written (as the _smooth entry).
 *   workspace  ..._fp8pv_workspace_bytes (with k_mean: ..._fp8pv_smooth_workspace_bytes) bytes, 16-byte aligned; no result depends on what it held.
 *
 * qattn_fp8_quant_attention_varlen_window_forward_fp8pv (qattn_window.h): every line of qattn_fp8_quant_attention_varlen_forward_fp8pv above --
 *   q8 / k8 / v8 / scale_q / scale_k / scale_v / k_mean  the same sizes, alignments and written bytes: the pre-pass is that entry's and covers ALL
 *              used keys, whatever the window leaves out.
 *   out / lse / row_path  every row of every sequence is written, rows whose window holds no key included (zeros / -inf / the tile's code).
 *   workspace  qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes (with k_mean: ..._fp8pv_smooth_workspace_bytes) bytes -- the packed
 *              FP8-PV entry's own two functions, there is no third --, 16-byte aligned; no result depends on what it held.
 *
 * qattn_rope_quant_qk_fp8 (qattn_rope.h; held by tests/test_gpu_rope_buffer_contract.py):
 *   q, k       [B,Hq,Sq,D] / [B,Hkv,Skv,D] 16-bit, dense or the 6-stride views of qattn_strided.h, 16-byte aligned; read: the D elements of each row.
 *   cos_*, sin_*  fp32, 16-byte aligned, rows read as float4: D/2 floats of each of the rows 0 .. S-1 of every batch element (batch stride 0: of
 *              the one table), row s at base + b batch_stride + s row_stride; S rows suffice -- no row is read for the padding rows of a ragged
 *              last 64-row tile, and no result depends on a byte outside those rows.
 *   q8         qattn_fp8_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, Sq, D) bytes, 16-byte aligned (8-byte stores); every byte written.
 *   k8         qattn_fp8_tensor_bytes(k_layout, B, Hkv, Skv, D) bytes, 16-byte aligned; every byte written, KFRAG: the zero padding up to 64 keys included.
 *   scale_q, scale_k  fp32 [B,H] or [B,H,S], 4-byte aligned; every element written.
 *   workspace  qattn_rope_quant_qk_workspace_bytes(B, Hq, Hkv) bytes, 4-byte aligned (head-wise scales; not touched with token-wise ones); no
 *              result depends on what it held.
 *
 * qattn_fp8_rope_quant_attention_forward (qattn_rope.h): q, k, tables, q8, k8 (KFRAG), scale_q, scale_k as above, all written;
 *   v          dense [B,Hkv,Skv,D] 16-bit, 16-byte aligned.
 *   v8         qattn_fp8_tensor_bytes(QATTN_LAYOUT_VFRAG, B, Hkv, Skv, D) bytes, 16-byte aligned, and scale_v fp32 [B,Hkv], 4-byte aligned: every
 *              byte / element written when v_fmt = fp8_fmt; not touched (may be NULL) with a 16-bit V.
 *   out        dense [B,Hq,Sq,D] in in_fmt, 16-byte aligned; lse (NULL or qattn_lse_row_stride floats per (b,h), 4-byte aligned): as
 *              qattn_fp8_attention_forward -- every element of out, the Sq floats of each lse row.
 *   workspace  qattn_fp8_rope_quant_attention_workspace_bytes(B, Hq, Hkv, Sq, Skv, D) bytes, 16-byte aligned; no result depends on what it held.
 *
 * qattn_fp8_attention_splitkv_forward (qattn_splitkv.h; held by tests/test_gpu_splitkv_buffer_contract.py), rows = B Hq Sq, ns = num_splits:
 *   q16        dense [B,Hq,Sq,D] 16-bit, 16-byte aligned; read: every element.
 *   k8_kfrag, v8_vfrag  qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG / _VFRAG, B, Hkv, Skv, D) bytes each, 16-byte aligned; read: of batch element b
 *              the 64-key chunks 0 .. ceil(L_b / 64) - 1 of every kv head (causal: up to the last chunk a row attends), no other byte.  In
 *              the chunk that holds key L_b the bytes of the keys >= L_b are read and influence no result, whatever they hold (NaN bytes
 *              included): K's scores are replaced by -inf, V's bytes are zeroed before the product.
 *   scale_k, scale_v  fp32 [B,Hkv], 4-byte aligned.   seqused_k: NULL or int32 [B], 4-byte aligned.
 *   out        dense [B,Hq,Sq,D] in in_fmt, 16-byte aligned; every element written (rows without a key: zeros).
 *   lse        NULL or fp32 [B,Hq,Sq], 4-byte aligned; every element written (rows without a key: -inf) -- except by a FAST call with ns = 1,
 *              whose one-term workgroups (byte exponentials) would not write theirs: FAST with lse != NULL runs exact exponentials instead.
 *   q8         NULL or qattn_fp8_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, Sq, D) bytes, 16-byte aligned; scale_q: NULL or fp32 [B,Hq], 4-byte
 *              aligned; row_path: NULL or uint8 [B,Hq,Sq], 1-byte aligned.  Every byte / element written.
 *   partial_o  NULL or fp32 [ns,B,Hq,Sq,D], 16-byte aligned; partial_lse: NULL or fp32 [ns,B,Hq,Sq], 4-byte aligned; partial_path: NULL or
 *              uint8 [ns,B,Hq,Sq], 1-byte aligned.  ns > 1: every element written (a split that gave a row no key: zeros, -inf,
 *              QATTN_PATH_ONE_TERM) and left as the sweep wrote it (the merge accumulates in the workspace).  ns = 1: not touched.
 *   workspace  qattn_fp8_attention_splitkv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D, num_splits) bytes (num_splits as passed: 0 sizes it for the most splits), 16-byte aligned, always needed (it holds
 *              whatever optional output is NULL, the pre-pass words and, for ns > 8, the merge's fp32 accumulator); no result depends on
 *              what it held.
 *
 * qattn_kv_cache_append_fp8 (qattn_kvcache.h; held by tests/test_gpu_kvcache_buffer_contract.py), p_b / n_b as the header defines them:
 *   k16, v16   [B,Hkv,T,D] 16-bit through the element strides {batch, head, token} of k_strides3 / v_strides3, head_dim innermost and dense;
 *              base 16-byte aligned, every stride a NON-NEGATIVE multiple of 8 elements (16-byte loads; anything else: QATTN_ERR_INVALID_ARG).  Read: the D elements of the rows of the tokens
 *              t < min(n_b, capacity - p_b) of batch element b, no other byte -- not the rows of dropped tokens, not the pads between rows.
 *   k8_kfrag, v8_vfrag  qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG / _VFRAG, B, Hkv, capacity, D) bytes each, 16-byte aligned.  Written: the D bytes
 *              of each of the keys p_b .. min(p_b + n_b, capacity) - 1 of every kv head of batch element b (16-byte, 8-byte, 4-byte and
 *              single-byte stores); every other byte -- other keys of the same chunk, the zero padding up to 64 keys -- keeps what it held.
 *              Never read: no result depends on what the images held.
 *   scale_k, scale_v  fp32 [B,Hkv], 4-byte aligned; read.
 *   seqlens    int32 [B], 4-byte aligned; read, and with advance != 0 every element rewritten (min(p_b + n_b, capacity): a value outside
 *              [0, capacity] comes back clamped); advance = 0: not written.   new_lens: NULL or int32 [B], 4-byte aligned; read.
 *   No workspace.
 *
 * qattn_paged_kv_cache_append_fp8 and qattn_fp8_attention_paged_splitkv_forward (qattn_paged.h; held by tests/test_gpu_paged_buffer_contract.py):
 * every line of qattn_kv_cache_append_fp8 / qattn_fp8_attention_splitkv_forward above with capacity = max_pages page_size, except
 *   k_pool, v_pool  qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG / _VFRAG, num_pages, Hkv, page_size, D) bytes each, 16-byte aligned, in place of
 *              k8_kfrag / v8_vfrag.  Append: written are the D bytes of each appended key, at key j % page_size of page
 *              clamp(block_table[b][j / page_size], 0, num_pages - 1); every other byte of the pool keeps what it held; never read.
 *              Attention: read are the chunks of the pages the table names for the chunks 0 .. ceil(L_b / 64) - 1 of sequence b
 *              (causal: up to the last chunk a row attends), no other byte; bytes behind L_b in the chunk that holds key L_b influence
 *              no result, as in the contiguous entry.
 *   block_table  int32 [B, max_pages] with a row stride of table_stride >= max_pages elements, 4-byte aligned; read: the entries of the
 *              pages that hold the appended keys / the chunks named above, no other entry; each clamped before it forms an address.
 *   seqused_k  int32 [B], 4-byte aligned, REQUIRED by the attention entry.
 *   workspace  qattn_fp8_attention_paged_splitkv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D, num_splits) bytes, 16-byte aligned (the append: none).
 *
 * qattn_fp8_attention_paged_varlen_forward (qattn_paged_varlen.h; held by tests/test_gpu_paged_varlen_buffer_contract.py): k_pool, v_pool,
 * block_table, scale_k, scale_v and seqused_k as the paged attention entry above (L_i, the entries and chunks read: per sequence i), and
 *   q16        [total_q, Hq, D] 16-bit through the element strides {token, head} of q_strides2 (NULL: dense), head_dim innermost and dense;
 *              base 16-byte aligned, both strides NON-NEGATIVE multiples of 8 elements.  Read: the D elements of each (token, head) row of
 *              the tokens that belong to a sequence, no other byte -- not the pads between rows or heads.
 *   cu_seqlens_q  int32 [B + 1], 4-byte aligned; read, every extent clamped into [0, total_q].
 *   out        dense [total_q, Hq, D] in in_fmt, 16-byte aligned.   lse: NULL or fp32 [Hq, total_q], 4-byte aligned (FAST with ns = 1: as the
 *              split-KV entry).   row_path: NULL or uint8 [Hq, total_q], 1-byte aligned.
 *   q8         NULL or Hq total_q D bytes, 16-byte aligned: sequence i's row-major [Hq, Sq_i, D] slab at byte Hq D start_i.   scale_q: NULL or
 *              fp32 [B, Hq], 4-byte aligned: every element written, an idle sequence's too.
 *   partial_o  NULL or fp32 [ns, total_q, Hq, D], 16-byte aligned; partial_lse: NULL or fp32 [ns, Hq, total_q], 4-byte aligned; partial_path:
 *              NULL or uint8 [ns, Hq, total_q], 1-byte aligned.  ns > 1: written and left as the sweep wrote them; ns = 1: not touched.
 *   written    of out, lse, row_path, q8 and the partials: every element of every token that belongs to a sequence (a row without a key:
 *              zeros, -inf, QATTN_PATH_ONE_TERM) -- with a consistent cu_seqlens_q whose last entry is total_q, every element.  The rows
 *              of tokens that belong to no sequence (cu_seqlens_q[B] < total_q) have unspecified contents: out, lse and row_path rows of
 *              such tokens are written by the merge with ns > 1 (from partials nobody wrote) and not at all with ns = 1.
 *   workspace  qattn_fp8_attention_paged_varlen_workspace_bytes(B, Hq, Hkv, total_q, Skv, D, num_splits) bytes (num_splits as passed: 0 sizes
 *              it for the most splits), 16-byte aligned, needed whenever total_q > 0 (total_q = 0: nothing is launched or written, the
 *              workspace's size is not looked at); it holds whatever optional output is NULL, the pre-pass's abs-max words and, for ns > 8, the merge's fp32 accumulator; no
 *              result depends on what it held.
 *
 * qattn_paged_kv_cache_append_varlen_fp8 (qattn_paged_varlen_append.h; held by tests/test_gpu_paged_varlen_append_buffer_contract.py): k_pool,
 * v_pool, block_table, scale_k, scale_v and seqlens as qattn_paged_kv_cache_append_fp8 above (per sequence i), and
 *   k16, v16   [total, Hkv, D] 16-bit through the element strides {token, head} of k_strides2 / v_strides2, head_dim innermost and dense;
 *              base 16-byte aligned, both strides NON-NEGATIVE multiples of 8 elements.  Exactly `total` rows: the last row's last element
 *              ends the buffer.  Read: the D elements of each (token, head) row of the tokens that are appended, no other byte -- not
 *              the pads between rows or heads, not the rows behind cu_seqlens[B], not a dropped token's.
 *   cu_seqlens  int32 [B + 1], 4-byte aligned; read, every extent clamped into [0, total].
 *   No workspace.
 *
 * qattn_paged_kv_cache_append_varlen_rope_fp8 and qattn_rope_paged_varlen (qattn_paged_varlen_rope.h; held by
 * tests/test_gpu_paged_varlen_rope_buffer_contract.py): no workspace.  The append: every line of qattn_paged_kv_cache_append_varlen_fp8
 * above -- the same bytes of k_pool and v_pool are written, those of the appended keys and no other, and seqlens with advance -- and
 *   cos, sin   fp32 [T, D/2] through table_row_stride floats (a non-negative multiple of 4), both bases 16-byte aligned.  Exactly T rows: the
 *              last row's last float ends the buffer.  Read: the D/2 floats of the rows min(p_i + t, T - 1) of the appended keys, no other
 *              byte -- not the pads between rows of a sliced table, not a row no appended key uses.
 * The rotation: x16 [total, H, D] as k16 above (exactly `total` rows; read: the rows a sequence owns, not those behind cu_seqlens[B]);
 * cos, sin as above (read: the rows min(max(base_i, 0) + t, T - 1)); cu_seqlens int32 [B + 1] and seqlens int32 [B], 4-byte aligned, read;
 *   out16      dense [total, H, D] in x16's dtype, 2 total H D bytes, 16-byte aligned.  Written: every element of the rows a sequence
 *              owns; the rows behind cu_seqlens[B] are not written.
 *
 * qattn_fp8_attention_splitkv_window_forward, qattn_fp8_attention_paged_splitkv_window_forward and
 * qattn_fp8_attention_paged_varlen_window_forward (qattn_splitkv_window.h; held by tests/test_gpu_splitkv_window_buffer_contract.py): every
 * line of the sibling without a window -- qattn_fp8_attention_splitkv_forward, qattn_fp8_attention_paged_splitkv_forward,
 * qattn_fp8_attention_paged_varlen_forward -- with window_left, window_right (two ints, no buffer) in is_causal's place, the same
 * sizes, alignments and written elements, and the sibling's own workspace size function.  What is READ shrinks: with
 * lo_i = window_left < 0 ? 0 : clamp(L_i - Sq_i - window_left, 0, L_i),
 *   k8 / v8, k_pool / v_pool  the 64-key chunks lo_i / 64 .. ceil(L_i / 64) - 1 of sequence i at the most (a tile: the chunks of the keys its
 *              rows attend), no other byte; the bytes of the keys below lo_i in lo_i's chunk and behind L_i in L_i's chunk are fetched and
 *              influence no result (NaN patterns included).
 *   block_table  the entries lo_i / page_size .. ceil(L_i / page_size) - 1 of row i at the most, each clamped before it forms an address;
 *              the leading entries may hold anything (their pages may have been handed to another sequence).
 */
#ifndef QATTN_BUFFERS_H_
#define QATTN_BUFFERS_H_
#include "qattn.h"
#endif /* QATTN_BUFFERS_H_ */
