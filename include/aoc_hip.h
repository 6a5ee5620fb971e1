/*
 * aoc_hip.h -- C ABI of libaoc_hip.so: the MI355X (gfx950) implementation of the AOC-Net
 * adaptive-proxy matching + mask-calibration hot path.
 *
 * The reference has no FFI layer; its operator surface is the set of Python functions that
 * aocnet.py:6-7 and decoding_module.py:4,7 import.  Each entry point below names the reference
 * code it replaces (paths relative to /root/reference/AOC-Net; AEM =
 * adaptive_embedding_for_matching.py == complete_project/AOCNet/networks/layers/matching.py,
 * ATT = complete_project/AOCNet/networks/layers/attention.py, CL = conditioning_layer.py).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer unless the name ends in _host;
 *  - all buffers (outputs and workspaces included) are caller-owned; nothing is allocated;
 *  - work is enqueued on `stream` (a hipStream_t passed as void*) and NOT synchronised;
 *  - return value: 0 = enqueued, < 0 = aoc_status error (nothing enqueued); never throws;
 *  - fp32 data, row-major; "rows" are pixels of stride-4 feature maps; C = embedding width.
 *
 * Workspaces
 *  A `workspace` argument may hold ANYTHING on entry -- another call's leftovers, another shape's, uninitialised memory -- unless the
 *  entry says otherwise: every entry initialises what it reads, and its results do not depend on what the bytes held
 *  (tests/test_gpu_carried_state.py runs each one in a zeroed workspace, in one of all-ones words and in one a larger case has just
 *  used, and wants the same bits).  A workspace is used by one stream at a time.  The entries that say otherwise:
 *   - aoc_proxy_corr_min_batched, aoc_proxy_corr_min_records, aoc_proxy_corr_min_records_cached: the take-over flag word is zeroed by
 *     the caller once after allocation and never reset; the cached form also keeps its pass tables there, described by *tables_key
 *     (0 = nothing cached: a workspace that is new, or was used for anything else, goes with a key of 0);
 *   - aoc_mask_jf_accumulate with workspace_is_clean != 0: the counters are zero on entry (the call leaves them zeroed);
 *   - aoc_dense_match_min_split_cached with reuse_plan != 0: the workspace holds what the last reuse_plan = 0 call for the same pool
 *     state and the same m left there, and nothing else has written to it since;
 *   - aoc_frame_enqueue: the workspace's content is described by the caller's aoc_seq_state; a zeroed state record goes with any content.
 *
 * Pointer alignment (label prep, k-means, proxy build, correlation, dense and local matching and their gradients, the frame and chain calls;
 * the entries further down state theirs in their own comments)
 *  Every device pointer is at least 4-byte aligned (float / int32 elements).  A pointer is CLASS 16 when some kernel reaches it through a
 *  16-byte access -- float4 / uint4 loads or stores, a 16-byte buffer load, an LDS-direct global_load_lds_dwordx4 -- or when it is an opaque
 *  record buffer of aoc_split_rows[_tiled]: it must lie on the 16-byte grid, and the entry returns AOC_ERR_INVALID_ARG for one that does
 *  not, BEFORE it enqueues or writes anything (host code: no kernel ever sees such a pointer).  With C a multiple of 4 every row of an
 *  aligned [*, C] table is aligned again, so pool prefixes, ref_emb[r] and table row ranges keep the class.  Every other pointer is CLASS 4:
 *  the kernels read and write it with 4-byte accesses only, and it may sit at any float boundary -- labels and bit masks, row lists,
 *  counts (counts + n_obj is what the library itself passes as n_fg), norms, biases, every `out` addressed with strides (a channel slice of
 *  the proto-mask tensor at odd hw), gradients.  No class-4 pointer's alignment enters a summation order: results do not depend on where
 *  it sits, bit for bit (tests/test_gpu_alignment.py).  HOST arrays and descriptors (*_host, frames_host, desc, state, tables_key) are read by
 *  the host code with their natural alignment; the classes of the pointers inside a descriptor are listed under the structure's name.
 *  tests/alignment_cases.py holds this table as data, with the source line behind every class-16 entry.  Class-16 pointers per entry
 *  (every pointer parameter not named is class 4; "-" = none):
 *   aoc_label_prep / aoc_label_bits                                         16: -
 *   aoc_kmeans_segmented / aoc_kmeans_segmented_ex / aoc_kmeans_segmented_rep   16: pool, centroids, workspace
 *   aoc_kmeans_replicate / aoc_kmeans_replicate_levels                      16: -
 *   aoc_build_proxies                                                       16: pool, workspace
 *   aoc_proxy_corr_min / aoc_proxy_corr_min_f16                             16: proxies
 *   aoc_proxy_corr_min_batched / aoc_proxy_corr_min_records                 16: -
 *   aoc_proxy_corr_min_records_cached                                       16: workspace
 *   aoc_corr_frame                                                          16: query, proxies
 *   aoc_corr_frame_rec                                                      16: query_rec, proxies
 *   aoc_dense_match_min / aoc_dense_match_min_f16 / aoc_dense_match_argmin  16: pool
 *   aoc_split_rows / aoc_split_rows_tiled                                   16: x, records
 *   aoc_dense_match_min_split / aoc_dense_match_min_split_cached            16: query, query_rec, pool, pool_rec, workspace
 *   aoc_dense_match_grad / aoc_proxy_match_grad                             16: -
 *   aoc_local_window_match / aoc_local_window_match_ex / aoc_local_window_match_argmin   16: query, prev
 *   aoc_local_window_match_pair                                             16: query, prev_a, prev_b
 *   aoc_local_match_grad / aoc_local_prep                                   16: -
 *   aoc_resize_bilinear_hwc / aoc_resize_bilinear_hwc_ex / aoc_resize_nearest_bits   16: -
 *   aoc_atrous_subsample                                                    16: in, out
 *   aoc_proxy_set_match_argmin / aoc_proxy_set_match_grad / aoc_centroid_avg_grad   16: -
 *   aoc_proto_finish / aoc_fg2bg_min                                        16: -
 *   aoc_frame_enqueue / aoc_cluster_chain_enqueue                           16: workspace
 *   aoc_frame_desc                                                          16: ref_emb, match_emb, prev_emb, cur_emb, proxy_table
 *   aoc_chain_desc                                                          16: pool, tables
 *  Two classes are conditional.  aoc_atrous_subsample: the class holds for X % 4 == 0, the one case that moves 16 bytes per thread; for every
 *  other X both pointers are class 4 and the entry accepts them anywhere.  aoc_proxy_corr_min_records_cached: the workspace is class 16 when
 *  tables_key != NULL (only then does it hold the tile tables, which have 8-byte members); with a NULL key the call is
 *  aoc_proxy_corr_min_records and the workspace class 4.  Each covered prototype below repeats its own line of this list.
 */
#ifndef AOC_HIP_H
#define AOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *aoc_stream_t; /* hipStream_t */

enum aoc_status {
    AOC_OK = 0,
    AOC_ERR_INVALID_ARG = -1,   /* null pointer, negative size, unsupported width ... */
    AOC_ERR_WORKSPACE = -2,     /* workspace smaller than aoc_*_workspace_bytes()       */
    AOC_ERR_LAUNCH = -3,        /* hipGetLastError() != hipSuccess after a launch        */
    AOC_ERR_UNSUPPORTED = -4    /* e.g. more than AOC_MAX_OBJECTS objects                */
};

#define AOC_MAX_OBJECTS 30          /* label bits live in a uint32 (bit 31 = "row kept")      */
#define AOC_MAX_CHANNELS 256        /* embedding width handled by the matching kernels         */
#define AOC_MAX_CLUSTERS 64         /* proxies per object per level (cfg4)                     */
#define AOC_PAD_DISTANCE 5.0e4f     /* WRONG_LABEL_PADDING_DISTANCE, AEM:25                    */
#define AOC_ROW_KEPT_BIT 0x80000000u

/* Library / build identification (string is static). */
const char *aoc_version(void);

/* ------------------------------------------------------------------------------------------
 * Label preparation.  Replaces the masked_select / nonzero / index_select plumbing of
 * AEM:197-198 (wrong-label mask, label < 0.1), AEM:252,263-264 (per-object rows, label > 0.9)
 * and AEM:585-591 (keep rows whose label sum > 0.9).  Nothing is copied: the reference pool
 * stays in place and later kernels gather rows through the index lists produced here.
 *
 *  labels      [n, n_obj] float            (the concatenated [h,w,O] label maps of the pool)
 *  right_bits  [n] out: bit o = label[j,o] > 0.9 ; bit 31 = row kept (sum_o label[j,o] > 0.9)
 *  wrong_bits  [n] out: bit o = label[j,o] < 0.1
 *  fg_rows     [n] out: pool row of every kept row, ascending (first counts[n_obj] valid)
 *  obj_rows    [n_obj * n] out: for object o, at obj_offsets[o], the pool rows that are kept
 *              AND right for o, ascending  (the reference's reference_embeddings_flat_cur)
 *  counts      [n_obj + 1] out: rows per object; counts[n_obj] = kept rows
 *  obj_offsets [n_obj + 1] out: exclusive prefix sum of counts[0..n_obj)
 */
size_t aoc_label_prep_workspace_bytes(int64_t n, int n_obj);
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_label_prep(const float *labels, int64_t n, int n_obj,
                   uint32_t *right_bits, uint32_t *wrong_bits,
                   int32_t *fg_rows, int32_t *obj_rows,
                   int32_t *counts, int32_t *obj_offsets,
                   void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* Bit masks only (same definition as above; wrong_bits may be NULL).  Used by local matching
 * (AEM:1023-1028: label > 0.9 of the previous frame). */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_label_bits(const float *labels, int64_t n, int n_obj, uint32_t *right_bits,
                   uint32_t *wrong_bits, aoc_stream_t stream);

/* Sticky cluster count of AEM:268 (the loop variable is overwritten): k[o] = min(k[o-1], counts[o]),
 * k[-1] = cluster_num.  Device-side so that a pipeline needs no host round trip. */
int aoc_kmeans_plan(const int32_t *counts, int n_seg, int cluster_num, int32_t *seg_k,
                    aoc_stream_t stream);

/* HOST function (no device work, no stream): the initial rows of the k-means calls of n_frames frames x n_levels levels x n_obj objects that see
 * one pool state, exactly as the reference draws them -- scipy kmeans2(minit='points') -> numpy.random.RandomState.choice(n, k, replace=False)
 * = permutation(n)[:k] on the global legacy MT19937 stream, in the order frame, level, object, with the sticky cluster count of AEM:268 and no
 * draw where it is zero (AEM:263-276).  mt_key [624] / *mt_pos: the generator's state (numpy get_state()[1:3]), advanced in place.
 * counts [n_obj] (host), levels [n_levels] (host, each <= kmax); rows_out [n_frames][n_levels * n_obj][kmax] int32 (host), unused entries 0;
 * states_out (may be NULL) [n_frames][625]: key + pos as each frame's first draw finds them (to hand unused frames' draws back). */
int aoc_kmeans_init_rows_draw(uint32_t *mt_key, int32_t *mt_pos, const int32_t *counts, int n_obj, const int32_t *levels, int n_levels,
                              int n_frames, int kmax, int32_t *rows_out, uint32_t *states_out);

/* Segment lists replicated n_rep times: the k-means of several frames that see the SAME pool (the reference re-clusters
 * the whole pool every frame with fresh initial rows, AEM:268-276; the pool only changes every MEM_EVERY frames,
 * eval_manager_mm.py:356-361) can then advance together in one aoc_kmeans_segmented_ex call with n_rep * n_seg segments.
 * rows_out [n_rep * rows_capacity], seg_offsets_out [n_rep * n_seg + 1], seg_k_out [n_rep * n_seg]; replica f's segment s
 * is rows_out[seg_offsets_out[f * n_seg + s] ...).  Device-side (the segment sizes never reach the host). */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_kmeans_replicate(const int32_t *rows, const int32_t *seg_offsets, const int32_t *seg_k, int n_seg, int n_rep,
                         int64_t rows_capacity, int32_t *rows_out, int32_t *seg_offsets_out, int32_t *seg_k_out,
                         aoc_stream_t stream);

/* The same with a cluster count per replica: replica f clusters with K = levels_host[f % n_levels], made sticky per replica from
 * the segment sizes exactly like aoc_kmeans_plan (AEM:268).  This is the multi-level configuration (BASELINE.json configs[2],
 * K in {8, 16, 32}; the reference's `cluster_num` argument, AEM:231-232, one call per level): n_rep = frames x levels replicas
 * advance in ONE aoc_kmeans_segmented_ex chain with kmax = max level.  n_levels <= 8.  n_rep == 1 with rows_out == rows only
 * writes seg_offsets_out / seg_k_out. */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_kmeans_replicate_levels(const int32_t *rows, const int32_t *seg_offsets, int n_seg, int n_rep,
                                const int32_t *levels_host, int n_levels, int64_t rows_capacity, int32_t *rows_out,
                                int32_t *seg_offsets_out, int32_t *seg_k_out, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segmented Lloyd k-means, bit-identical to scipy.cluster.vq.kmeans2(X, K, minit='matrix',
 * iter=iters) as called at AEM:276 (one "segment" = one object's rows; all segments advance in
 * the same launches).  Arithmetic order is scipy's (see oracle/csrc/aoc_oracle.c): sequential
 * mul-then-add row norms, one k-ordered fma chain per dot product, (M + |x|^2) + |c|^2, strict <
 * (ties -> lowest index), per-cluster sums in row order, division by (float)count, empty cluster
 * keeps its centroid.
 *
 *  pool         [*, C]        embeddings the row ids refer to (pool_rows of them in the _ex form: a segment lists DISTINCT
 *                             pool rows, so no segment is longer than pool_rows -- the per-segment grids rely on it)
 *  rows         packed row ids (aoc_label_prep's obj_rows); segment s = rows[seg_offsets[s] .. seg_offsets[s+1])
 *  seg_offsets  [n_seg + 1]   device
 *  seg_k        [n_seg]       device; 0 = segment skipped (reference: centroid None, AEM:271-273)
 *  init_rows    [n_seg, kmax] device; segment-local indices of the initial centroids
 *                             (scipy minit='points': permutation(n_i)[:K_i])
 *  rows_capacity              host-known upper bound of seg_offsets[n_seg] (sizes the grids)
 *  centroids    [n_seg, kmax, C] out   final code book
 *  labels       [rows_capacity]  out   segment-local cluster id of every packed row (last assignment)
 *  cluster_counts [n_seg, kmax]  out   members per cluster in the last update
 * Slots j >= seg_k[s] (every slot of a skipped segment) come back as zero centroids and zero counts; the labels of a skipped
 * segment are not written.  An init_rows entry outside its segment is clamped into it.
 */
size_t aoc_kmeans_workspace_bytes(int64_t rows_capacity, int n_seg, int kmax, int C);
/* Same, with the number of rows of `pool` stated (pool_rows > 0): enables the pipelined ordered
 * accumulation, which addresses rows through a bounds-checked buffer descriptor.  pool_rows = 0
 * (or aoc_kmeans_segmented) selects the generic path.  Results are bit-identical either way. */
/* Alignment ("Pointer alignment" above): class 16: pool, centroids, workspace; every other pointer class 4. */
int aoc_kmeans_segmented_ex(const float *pool, int64_t pool_rows, int C,
                            const int32_t *rows, const int32_t *seg_offsets, const int32_t *seg_k,
                            const int32_t *init_rows, int n_seg, int kmax, int iters,
                            int64_t rows_capacity,
                            float *centroids, int32_t *labels, int32_t *cluster_counts,
                            void *workspace, size_t workspace_bytes, aoc_stream_t stream);
/* The same for REPLICATED segment lists (aoc_kmeans_replicate / aoc_kmeans_replicate_levels): n_seg = n_rep * n_base segments, segment
 * f * n_base + s lists the same rows, in the same order, as segment s (initial rows and cluster counts differ).  That is the k-means of
 * several frames that see one pool state (AEM:268-276, eval_manager_mm.py:356-361) and of the cluster levels of BASELINE.json configs[2]
 * in ONE chain; stating n_rep lets the assignment step fetch every pool row once per group of replicas instead of once per replica.
 * Results are bit-identical to n_rep = 1 (= aoc_kmeans_segmented_ex), which is always a valid way to run the same lists. */
/* Alignment ("Pointer alignment" above): class 16: pool, centroids, workspace; every other pointer class 4. */
int aoc_kmeans_segmented_rep(const float *pool, int64_t pool_rows, int C,
                             const int32_t *rows, const int32_t *seg_offsets, const int32_t *seg_k,
                             const int32_t *init_rows, int n_seg, int n_rep, int kmax, int iters,
                             int64_t rows_capacity,
                             float *centroids, int32_t *labels, int32_t *cluster_counts,
                             void *workspace, size_t workspace_bytes, aoc_stream_t stream);
/* Alignment ("Pointer alignment" above): class 16: pool, centroids, workspace; every other pointer class 4. */
int aoc_kmeans_segmented(const float *pool, int C,
                         const int32_t *rows, const int32_t *seg_offsets, const int32_t *seg_k,
                         const int32_t *init_rows, int n_seg, int kmax, int iters,
                         int64_t rows_capacity,
                         float *centroids, int32_t *labels, int32_t *cluster_counts,
                         void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The reference's second proxy set, AEM:280: for every non-empty cluster j of segment s the mean of
 * the rows  fg[p], p in {segment-local indices with label == j}  of the GLOBAL kept-row array (the
 * reference indexes the wrong array; reproduced as is).  Also emits the squared norms of both
 * proxy sets (AEM:282); an empty / absent proxy gets norm = +inf so that a min skips it.
 *
 *  proxies      [n_seg, 2, kmax, C] out : [:,0] = centroids (copied), [:,1] = centroid_avg
 *  proxy_sqnorm [n_seg, 2, kmax]   out
 */
size_t aoc_build_proxies_workspace_bytes(int64_t rows_capacity, int n_seg, int kmax);
/* Alignment ("Pointer alignment" above): class 16: pool, workspace; every other pointer class 4. */
int aoc_build_proxies(const float *pool, int64_t pool_rows, int C, const int32_t *fg_rows,
                      const int32_t *seg_offsets, const int32_t *seg_k, const int32_t *labels,
                      const float *centroids, int n_seg, int kmax, int64_t rows_capacity,
                      float *proxies, float *proxy_sqnorm,
                      void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pixel-to-proxy correlation ("the correlation kernel"): AEM:92-110 + 316-319 (min over an
 * object's adaptive proxies), AEM:112-128 (k = 1 proxies, no min), fused with the proto-mask
 * transform (sigmoid(d + bias) - 0.5) * 2 of AEM:393/602/864.
 *
 *  query        [m, C]
 *  proxies      [n_proxy, C], proxy_sqnorm [n_proxy] (+inf = ignore; NULL = computed in-kernel)
 *  sets         HOST arrays of length n_set: set s = proxies[set_begin[s] .. set_begin[s] + set_size[s]);
 *               value = min over the set; an empty or all-ignored set yields AOC_PAD_DISTANCE
 *               (reference: absent object, AEM:310-313).  Single-proxy sets are the k = 1 proxies
 *               (no min; one whose norm is +inf is an all-ignored set like any other).  The set
 *               structure is static (kmax slots per object; unused slots carry norm = +inf), so the
 *               host knows it without a device round trip.
 *  set_bias     [n_set] device (dis_bias of the set's object); may be NULL (= 0)
 *  out element (pixel i, set s) is written at out[i * out_pixel_stride + set_out_offset[s]], so a set
 *               can land in its channel of the [O, 24, h, w] proto-mask buffer or in [1,h,w,O,F].
 *  transform    1 = apply the proto-mask transform, 0 = raw squared distance
 */
/* Alignment ("Pointer alignment" above): class 16: proxies; every other pointer class 4. */
int aoc_proxy_corr_min(const float *query, int64_t m, int C,
                       const float *proxies, const float *proxy_sqnorm, int n_proxy,
                       int n_set, const int32_t *set_begin_host, const int32_t *set_size_host,
                       const int64_t *set_out_offset_host, const float *set_bias,
                       float *out, int64_t out_pixel_stride, int transform, aoc_stream_t stream);

/* use_float16=True (AEM:388-392 / matching.py:2640-2646: `.half()` operands): same arguments; operands, |q|^2, |p|^2, the dot products and
 * the distances are rounded to float16 where the reference's float16 tensors round them (sums accumulate in fp32, as torch does);
 * proxy_sqnorm is only consulted for its +inf "absent" marks.  Outputs are fp32 (the bias is added and the sigmoid taken in fp32, as the
 * reference's type promotion does). */
/* Alignment ("Pointer alignment" above): class 16: proxies; every other pointer class 4. */
int aoc_proxy_corr_min_f16(const float *query, int64_t m, int C,
                           const float *proxies, const float *proxy_sqnorm, int n_proxy,
                           int n_set, const int32_t *set_begin_host, const int32_t *set_size_host,
                           const int64_t *set_out_offset_host, const float *set_bias,
                           float *out, int64_t out_pixel_stride, int transform, aoc_stream_t stream);

/* Batched form: the same correlation for n_frames frames (of one or of several independent sequences) in ONE persistent launch.
 * One 480p frame is 11.6 MB of traffic: a launch that small is latency-bound by construction ("tiny working sets"), and
 * the reference runs 2 x O x n_chunks launches per frame (AEM:316-319).  All frames share m, C and the set structure (same number
 * of objects and proxy levels); their pointers differ.  Outputs are pixel-contiguous planes: element (pixel i, set s) of frame f is
 * written at frames[f].out[set_out_offset[s] + i].
 *
 *  precision AOC_CORR_SPLIT (C = 100 only; other widths run the fp32 kernel): every value x 2^10 is split in registers into hi + lo
 *            fp16 and q.p = qh.ph + qh.pl + ql.ph (dropped ql.pl term < 2^-22 |q.p|) is accumulated in fp32 by
 *            v_mfma_f32_32x32x16_f16 as ONE K = 304 dot product that also carries -|p|^2/2; fp32-equivalent: tests/test_gpu_global_match.py
 *            holds raw and transformed outputs to a float64 reference under a bound that evaluates the split of every operand and
 *            adds gamma(337) for the accumulation (tests/global_match_bounds.py: about 1e-5 on distances of O(1)).
 *            Needs |x| 2^10 <= 65000 and |x|^2 <= 4000 for every query / proxy value; checked on the device, and when it
 *            fails the exact-fp32 kernel recomputes the launch inside the same call (no host round trip).
 *  precision AOC_CORR_FP32: exact fp32 MFMA (v_mfma_f32_16x16x4_f32), the arithmetic of aoc_proxy_corr_min.
 *  workspace: aoc_proxy_corr_min_batched_workspace_bytes() bytes (the device-side take-over flag: the kernel stores the call's sequence
 *            number there when a precondition fails and the gated fp32 kernel runs iff it finds it).  Zero it once after allocation and
 *            use it from one stream at a time; the calls themselves never reset it. */
/* Alignment ("Pointer alignment" above): class 16: query, proxies; every other pointer class 4. */
typedef struct aoc_corr_frame {
    const float *query;         /* [m, C] */
    const float *proxies;       /* [n_proxy, C] */
    const float *proxy_sqnorm;  /* [n_proxy] (+inf = ignore) or NULL */
    const float *set_bias;      /* [n_set] or NULL */
    float *out;
} aoc_corr_frame;
enum aoc_corr_precision { AOC_CORR_SPLIT = 0, AOC_CORR_FP32 = 1 };
size_t aoc_proxy_corr_min_batched_workspace_bytes(void);
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_proxy_corr_min_batched(const aoc_corr_frame *frames_host, int n_frames, int64_t m, int C, int n_proxy, int n_set,
                               const int32_t *set_begin_host, const int32_t *set_size_host,
                               const int64_t *set_out_offset_host, int transform, int precision,
                               void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The same correlation (AEM:92-128 + 316-319, proto-mask transform of AEM:393/602/864) with the query side handed over as the
 * tile-major fp16 split records of aoc_split_rows_tiled -- what the dense kernel consumes for the same frame (aoc_dense_match_min_split
 * with query_rec_tiled = 1), so a frame's query is converted once and both kernels stream it in their MFMA operand layout.  Always the
 * fp16-split arithmetic (C = 100) with the same device-side take-over by the exact-fp32 kernel (which reads `query`); results equal
 * aoc_proxy_corr_min_batched(precision = AOC_CORR_SPLIT) up to the summation order of |q|^2 (query_sqnorm is the sequential sum).
 * Same workspace as aoc_proxy_corr_min_batched. */
/* Alignment ("Pointer alignment" above): class 16: query_rec, proxies; every other pointer class 4. */
typedef struct aoc_corr_frame_rec {
    const float *query;         /* [m, C] fp32 rows (take-over only) */
    const void *query_rec;      /* aoc_split_rows_tiled(query) */
    const float *query_sqnorm;  /* [m], from the same call */
    const float *proxies;       /* [n_proxy, C] */
    const float *proxy_sqnorm;  /* [n_proxy] (+inf = ignore) or NULL */
    const float *set_bias;      /* [n_set] or NULL */
    float *out;
} aoc_corr_frame_rec;
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_proxy_corr_min_records(const aoc_corr_frame_rec *frames_host, int n_frames, int64_t m, int C, int n_proxy, int n_set,
                               const int32_t *set_begin_host, const int32_t *set_size_host,
                               const int64_t *set_out_offset_host, int transform,
                               void *workspace, size_t workspace_bytes, aoc_stream_t stream);
/* The same call as ONE launch whatever the number of proxy tiles (round 5).  A workgroup's LDS image holds 5 proxy tiles of 32 rows; a frame
 * with more (multi-level proxies: cfg3 has 22 tiles, cfg4 37) is cut into passes, and aoc_proxy_corr_min_records launches them one after
 * another -- ~30-40 us each for ~2 us of MFMA work (launch, image staging, one stream over the query records).  Here the passes are a grid
 * dimension: they run side by side and take the time of one.  Their tile tables live in the workspace
 * (aoc_proxy_corr_min_records_cached_workspace_bytes) and are rewritten only when *tables_key -- a caller-owned HOST word, 0 = nothing
 * cached, one per workspace -- does not match the call's set structure (a sequence writes them once).  tables_key = NULL: the plain call.
 * Results are identical to aoc_proxy_corr_min_records (every workgroup runs the same code on the same pass). */
size_t aoc_proxy_corr_min_records_cached_workspace_bytes(void);
/* Alignment ("Pointer alignment" above): class 16: workspace; every other pointer class 4. */
int aoc_proxy_corr_min_records_cached(const aoc_corr_frame_rec *frames_host, int n_frames, int64_t m, int C, int n_proxy, int n_set,
                                      const int32_t *set_begin_host, const int32_t *set_size_host,
                                      const int64_t *set_out_offset_host, int transform,
                                      void *workspace, size_t workspace_bytes, int64_t *tables_key, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dense pixel-level matching: AEM:178-227 + 61-89 without materialising [m, O, n]:
 *   out[i,o] = min_j ( (|q_i|^2 + |r_j|^2) - 2 q_i.r_j + 5e4 * wrong[j,o] ),  j over kept rows,
 * fused with the proto-mask transform (AEM:808).  fp32 MFMA (v_mfma_f32_16x16x4_f32).
 *
 *  pool [*, C]; fg_rows [n_fg_capacity] kept rows; n_fg device scalar (counts[n_obj] of label prep);
 *  wrong_bits [pool rows]; out element (i,o) at out[i*out_pixel_stride + o*out_obj_stride].
 *  n_fg == 0 yields 1.0 everywhere when transform != 0 (AEM:796-797), +inf otherwise.
 */
size_t aoc_dense_match_workspace_bytes(int64_t m, int64_t n_fg_capacity, int n_obj);
/* Alignment ("Pointer alignment" above): class 16: pool; every other pointer class 4. */
int aoc_dense_match_min(const float *query, int64_t m, int C,
                        const float *pool, const int32_t *fg_rows, const int32_t *n_fg,
                        int64_t n_fg_capacity, const uint32_t *wrong_bits,
                        const float *obj_bias, int n_obj,
                        float *out, int64_t out_pixel_stride, int64_t out_obj_stride,
                        int transform, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* use_float16=True (AEM:801-803 `.half()`; AEM:65-66 the wrong-label mask becomes float16 too): same arguments and workspace as
 * aoc_dense_match_min; operands, norms, dot products, distances, the 5e4 padding (49984 in float16) and its sum are rounded to float16
 * where the reference's float16 tensors round them (sums accumulate in fp32).  Outputs are fp32. */
/* Alignment ("Pointer alignment" above): class 16: pool; every other pointer class 4. */
int aoc_dense_match_min_f16(const float *query, int64_t m, int C,
                            const float *pool, const int32_t *fg_rows, const int32_t *n_fg,
                            int64_t n_fg_capacity, const uint32_t *wrong_bits,
                            const float *obj_bias, int n_obj,
                            float *out, int64_t out_pixel_stride, int64_t out_obj_stride,
                            int transform, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-time global matching (csrc/match_grad.hip): what autograd needs of global_matching (AEM:616-685 over AEM:178-227, 61-89) and
 * global_matching_proxy (AEM:336-402 over AEM:112-175) without the [m, O, n] distance tensor the reference keeps for its backward.
 * fp32 only.  With d = |q|^2 + |r|^2 - 2 q.r and T = 2 sigmoid(d + b) - 1:  dT/dd = dT/db = (1 - T^2) / 2, dd/dq = 2 (q - r*),
 * dd/dr* = 2 (r* - q), r* the row of the minimum (AEM:88 torch.min; the lowest row on ties).
 *
 * aoc_dense_match_argmin: aoc_dense_match_min (AEM:178-227 + 61-89, transform AEM:676) that also reports the minimiser.  Same arguments
 * plus arg, int32, addressed like out: arg[i*out_pixel_stride + o*out_obj_stride] = the POOL ROW (not the position in fg_rows) of the
 * minimum; ties go to the lowest pool row; -1 where the winning distance is a padded one (>= AOC_PAD_DISTANCE / 2: no right row) and
 * when *n_fg == 0 -- T is exactly 1.0f there and the gradient zero.  out holds bit for bit the values of aoc_dense_match_min (the same
 * tile routine; an index rides beside each minimum).  1 .. AOC_MAX_OBJECTS objects, C as aoc_dense_match_min. */
size_t aoc_dense_match_argmin_workspace_bytes(int64_t m, int64_t n_fg_capacity, int n_obj);
/* Alignment ("Pointer alignment" above): class 16: pool; every other pointer class 4. */
int aoc_dense_match_argmin(const float *query, int64_t m, int C,
                           const float *pool, const int32_t *fg_rows, const int32_t *n_fg,
                           int64_t n_fg_capacity, const uint32_t *wrong_bits,
                           const float *obj_bias, int n_obj,
                           float *out, int32_t *arg, int64_t out_pixel_stride, int64_t out_obj_stride,
                           int transform, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The backward of AEM:671-676 (min over the padded distances, proto-mask transform).  grad_out, T (the saved transformed output) and arg
 * (aoc_dense_match_argmin's) are addressed as [i*pixel_stride + o*obj_stride]; query [m, C]; pool [n, C], all n rows.
 *   g[i,o] = grad_out * 0.5 * (1 - T*T)
 *   grad_query [m, C]  = sum_o g * 2 (q_i - pool[arg])                     (pairs with arg < 0 or >= n contribute nothing)
 *   grad_pool  [n, C]  = sum over the pairs that chose the row of g * 2 (pool[r] - q_i); every row is written, rows nobody chose with zeros
 *   grad_bias  [n_obj] = sum_i g
 * Each output may be NULL (not wanted; nothing is written or computed for it).  Deterministic: no float atomics; every sum is added in a
 * fixed order (ascending pixel, then object; long lists over a fixed tree of pair-id ranges), so the same buffers give the same bits.
 * C <= AOC_MAX_CHANNELS, n_obj <= AOC_MAX_OBJECTS. */
size_t aoc_dense_match_grad_workspace_bytes(int64_t m, int64_t n, int C, int n_obj);
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_dense_match_grad(const float *grad_out, const float *T, const int32_t *arg, int64_t pixel_stride, int64_t obj_stride,
                         const float *query, int64_t m, int C, const float *pool, int64_t n, int n_obj,
                         float *grad_query, float *grad_pool, float *grad_bias,
                         void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The backward of the k = 1 proxy path (AEM:388-393: one distance per object, no min): the forward is aoc_proxy_corr_min with
 * single-proxy sets and transform = 1.  proxies [n_obj, C]; g as above;
 *   grad_query [m, C]       = sum_o g * 2 (q_i - p_o)
 *   grad_proxies [n_obj, C] = 2 (p_o sum_i g - sum_i g q_i)                (a two-stage reduction over the pixels in a fixed order)
 *   grad_bias [n_obj]       = sum_i g
 * Each output may be NULL.  Deterministic like aoc_dense_match_grad. */
size_t aoc_proxy_match_grad_workspace_bytes(int64_t m, int C, int n_obj);
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_proxy_match_grad(const float *grad_out, const float *T, int64_t pixel_stride, int64_t obj_stride,
                         const float *query, int64_t m, int C, const float *proxies, int n_obj,
                         float *grad_query, float *grad_proxies, float *grad_bias,
                         void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dense pixel-level matching on the fp16 matrix pipe with fp32-equivalent products (same reference
 * lines as aoc_dense_match_min).  Each embedding row is converted ONCE into a "split record":
 * x * 2^10 = hi + lo with hi, lo fp16 (two 11-bit significands: |error| <= 2^-22 |x|, typically 2^-23), plus the three fp16 pieces of -16 |x|^2 in
 * spare k-slots (and, in a fourth one, an upper bound of the norm of the row's lo plane).  q.r is then qh.rh + qh.rl + ql.rh
 * accumulated in fp32 by v_mfma_f32_32x32x16_f16 (the dropped ql.rl term is < 2^-22 |q| |r|): a product carries up to about 4x the
 * rounding error of an fp32 product, and the deviations of the min-distances from the fp32 reference stay within a small multiple
 * of the reference's own fp32 rounding (a few 1e-7 on distances of O(1)).  tests/test_gpu_global_match.py holds raw and transformed
 * outputs to a float64 reference under a bound that evaluates the split of every operand and the norm pieces and adds gamma(337) for the
 * accumulation (tests/global_match_bounds.py: about 2e-5 on distances of O(1)).
 *
 * The kernel evaluates the qh.rh product for every (32 reference pixels x 32 query pixels) pair and the two cross products only for
 * the pairs that can hold a minimum: |qh.rl + ql.rh| <= |qh||rl| + |ql||rh| (plane norms from the records), so a pair whose one-product
 * value lies further than that margin from the best three-product value already known for its (query pixel, object) is skipped.  The
 * minimum always survives and its value does not depend on what else was evaluated: same result as evaluating all three products
 * everywhere, run after run (tests/test_gpu_dense_split.py), at about 40 % of the matrix instructions.
 *
 * The fast kernels need (a) every |x| * 2^10 <= 65000 and |x|^2 <= 4000 and (b) every kept pool row right
 * for exactly one object (one-hot labels, as in the reference's eval loop).  Both are checked on the
 * device; when either fails the SAME call runs the exact-fp32 kernels of aoc_dense_match_min instead, on
 * the same stream, with no host round trip -- results are then bit-identical to aoc_dense_match_min.
 *
 *  aoc_split_record_bytes(C)   bytes per record (448) or 0 when C is unsupported (C % 4 != 0 or C > 100)
 *  aoc_split_rows              x [n, C] -> records [n * record_bytes], sqnorm [n] (may be NULL);
 *                              *overflow_flag |= 1 when a value does not fit (flag is sticky, caller zeroes it)
 *  aoc_split_rows_tiled        the same 16-byte chunks in tile-major order: per 32-row tile, per plane (hi, lo), per k-step the
 *                              64 chunks [k-half][row % 32] -- one coalesced 1 KiB wave load per MFMA B operand.  The buffer
 *                              holds whole tiles (aoc_split_rows_tiled_bytes(n, C)); rows past n are zero records.
 *  aoc_dense_match_min_split   query/pool [*, C] fp32 (only read by the fp32 take-over), query_rec/pool_rec
 *                              their records (query_rec_tiled != 0: query_rec is tile-major; the pool's are always row-major),
 *                              query_sqnorm [m]; n = pool rows; right_bits, wrong_bits, fg_rows,
 *                              obj_rows, counts, obj_offsets as produced by aoc_label_prep on the n pool rows;
 *                              out / strides / transform as aoc_dense_match_min.  n_obj <= 16.
 */
size_t aoc_split_record_bytes(int C);
/* Alignment ("Pointer alignment" above): class 16: x, records; every other pointer class 4. */
int aoc_split_rows(const float *x, int64_t n, int C, void *records, float *sqnorm,
                   int32_t *overflow_flag, aoc_stream_t stream);
size_t aoc_split_rows_tiled_bytes(int64_t n, int C);
/* Alignment ("Pointer alignment" above): class 16: x, records; every other pointer class 4. */
int aoc_split_rows_tiled(const float *x, int64_t n, int C, void *records, float *sqnorm,
                         int32_t *overflow_flag, aoc_stream_t stream);
size_t aoc_dense_match_split_workspace_bytes(int64_t m, int64_t n, int n_obj);
/* Alignment ("Pointer alignment" above): class 16: query, query_rec, pool, pool_rec, workspace; every other pointer class 4. */
int aoc_dense_match_min_split(const float *query, const void *query_rec, const float *query_sqnorm, int query_rec_tiled,
                              int64_t m, int C, const float *pool, const void *pool_rec,
                              const int32_t *overflow_flag, int64_t n,
                              const uint32_t *right_bits, const uint32_t *wrong_bits,
                              const int32_t *fg_rows, const int32_t *obj_rows,
                              const int32_t *counts, const int32_t *obj_offsets,
                              const float *obj_bias, int n_obj,
                              float *out, int64_t out_pixel_stride, int64_t out_obj_stride,
                              int transform, void *workspace, size_t workspace_bytes, aoc_stream_t stream);
/* The same call for a caller that keeps `workspace` across the frames that see ONE pool state (same pool rows, labels and records):
 * reuse_plan = 0 builds the plan (object-pure tile lists, norm maxima, one-hot check: a function of the pool alone) and leaves it in the
 * workspace; reuse_plan = 1 skips the plan kernel and both memsets (the finalize kernel of every call leaves the per-pixel bounds zeroed)
 * and only refreshes the gate from the sticky overflow flag.  Results are always within the bound of aoc_dense_match_min_split, and
 * identical to it bit for bit while the gate kept in the workspace agrees with the one that call would compute (the one case where it
 * does not: the first item below).
 * What a reusing call may assume of the call before it in the same workspace (tests/test_gpu_carried_state.py):
 *  - after a take-over frame (the overflow flag was raised, or the plan's one-hot check failed): every split kernel, the finalize
 *    kernel included, returned at the gate, so the per-pixel bounds are still the zeros the frame found.  The gate itself stays set
 *    in the workspace even if the caller clears the flag: every later reusing call is answered by the exact-fp32 kernels (correct,
 *    bit-identical to aoc_dense_match_min) until a reuse_plan = 0 call, made with the flag cleared, builds the plan again;
 *  - after a frame with n_fg = 0 (counts all zero): the plan has no tile, nothing was written to the bounds, the output was the
 *    constant (1.0 transformed, +inf raw); reusing calls give the same while the pool state stands;
 *  - an object with counts[o] = 0 has a bounds column that no kernel reads or writes: it keeps the zeros of the build;
 *  - m, n, n_obj and C are those of the build (they place the plan inside the workspace); a new pool state, of any size that fits,
 *    starts with reuse_plan = 0 in the same bytes. */
/* Alignment ("Pointer alignment" above): class 16: query, query_rec, pool, pool_rec, workspace; every other pointer class 4. */
int aoc_dense_match_min_split_cached(const float *query, const void *query_rec, const float *query_sqnorm, int query_rec_tiled,
                              int64_t m, int C, const float *pool, const void *pool_rec,
                              const int32_t *overflow_flag, int64_t n,
                              const uint32_t *right_bits, const uint32_t *wrong_bits,
                              const int32_t *fg_rows, const int32_t *obj_rows,
                              const int32_t *counts, const int32_t *obj_offsets,
                              const float *obj_bias, int n_obj,
                              float *out, int64_t out_pixel_stride, int64_t out_obj_stride,
                              int transform, void *workspace, size_t workspace_bytes, int reuse_plan, aoc_stream_t stream);

/* Developer counters of the coarse-then-rescore kernel behind aoc_dense_match_min_split, summed over all launches of the process
 * since the last reset (synchronises the device): out4[0] (reference tile, query tile) pairs tested with one fp16 product,
 * out4[1] pairs rescored with all three products, out4[2] reference tiles with at least one rescoring, out4[3] reference tiles. */
int aoc_dense_prune_stats(uint64_t *out4, int reset);
/* The same counters; out8[4..7] reserved (0). */
int aoc_dense_prune_stats_ex(uint64_t *out8, int reset);

/* How many CUs the streams that launch the matrix kernels (dense matching, batched correlation) may use -- a caller that runs them under a
 * HIP CU mask says so here and the kernels size their grids in whole rounds of that many CUs; 0 (default) = every CU of the device.
 * Process-wide, may be changed between calls.  (The library itself never reads the environment.) */
int aoc_set_stream_cus(int n_cus);

/* The dense share.  The matrix kernel of aoc_dense_match_min_split runs as G RESIDENT workgroups, one per CU, that walk the work list of
 * (512-pixel query block, tile split) items; G = the stream's CU budget (aoc_set_stream_cus / aoc_frame_desc.stream_cus, else 256) times
 * share_256 / 256, rounded down to a multiple of 8 (from 8 up), at least 1, at most the number of items.  The CUs it leaves out stay
 * free, for the whole launch, for what other streams enqueue (a resident dense workgroup fills a CU: nothing else runs beside it).  The
 * split count is chosen for G: the splits that fill whole rounds of G best, over up to three rounds (two at share 256, the rule of the
 * one-workgroup-per-item kernel).  Results do not depend on the share, bit for bit.
 * share_256 in 1 .. 256; process-wide, may be changed between calls; never read from the environment.  AOC_DENSE_SHARE_DEFAULT is what
 * a process starts with (DESIGN.md section 4.4 has the sweep that chose it). */
#define AOC_DENSE_SHARE_DEFAULT 224
int aoc_set_dense_share(int share_256);
int aoc_dense_share(void);
/* The sizing above as a function: m query pixels, budget CUs (0 = 256), share_256 -> the split count, the items (query blocks x
 * splits) and the resident workgroups G of the launch. */
int aoc_dense_split_sizing(int64_t m, int budget, int share_256, int32_t *splits, int32_t *items, int32_t *workgroups);

/* Measurement probe: the NEXT aoc_dense_match_min / aoc_dense_match_min_split call made by the calling thread records
 * `start` immediately before and `stop` immediately after its matrix kernel (dense_match_partial_kernel /
 * dense_prune_kernel) on the call's stream, then the probe is cleared.  Both are hipEvent_t created by the caller
 * (bench.py uses it to time that one kernel live, next to the rocprofv3 figure).  NULL, NULL disarms. */
int aoc_dense_match_set_probe(void *start_event, void *stop_event);

/* ------------------------------------------------------------------------------------------
 * Local (windowed) matching: AEM:921-963 + 968-1060 (and the identical local_matching_proxy,
 * AEM:1064-1156) without the F.unfold materialisation.  Works on maps already at matching
 * resolution (the bilinear down / up-sampling of AEM:938-941,1054-1056 are aoc_resize_*).
 *
 *  query, prev   [H, W, C]       right_bits [H*W] (bit o = prev label > 0.9 at that pixel)
 *  window radii  radii_host[n_radii] ascending, radii_host[n_radii-1] = max_distance (atrous 1)
 *  out           [n_obj, n_radii, H, W]; channel order [max, r_0, r_1, ...] (AEM:1034-1046);
 *                value = transform(min over the window of masked distances; 5e4 if none)
 */
/* Alignment ("Pointer alignment" above): class 16: query, prev; every other pointer class 4. */
int aoc_local_window_match(const float *query, const float *prev, const uint32_t *right_bits,
                           int H, int W, int C, const int32_t *radii_host, int n_radii,
                           const float *obj_bias, int n_obj, float *out, int transform,
                           aoc_stream_t stream);

/* The same with the two remaining arguments of the reference call (AEM:968-971):
 *   atrous_rate  window offsets are the multiples of the rate up to pad = max - max % rate (AEM:949-959 unfold with that stride); the
 *                nested windows are radii / rate rings (AEM:1039);
 *   float16      use_float16=True (AEM:1002-1005): operands, norms, dot products and distances are rounded to float16 exactly where the
 *                reference's float16 tensors round them (the sums accumulate in fp32 as torch does); outputs are fp32. */
/* Alignment ("Pointer alignment" above): class 16: query, prev; every other pointer class 4. */
int aoc_local_window_match_ex(const float *query, const float *prev, const uint32_t *right_bits,
                              int H, int W, int C, const int32_t *radii_host, int n_radii,
                              const float *obj_bias, int n_obj, float *out, int transform,
                              int atrous_rate, int float16, aoc_stream_t stream);

/* Bilinear (align_corners=True) resize of a channel-last map [h,w,C] -> [H,W,C]  (AEM:938-941).  _ex with float16 != 0: the resize
 * of a float16 tensor (float16 samples, fp32 arithmetic, float16 result), as F.interpolate does in the use_float16 mode. */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_resize_bilinear_hwc(const float *in, int h, int w, int C, float *out, int H, int W,
                            aoc_stream_t stream);
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_resize_bilinear_hwc_ex(const float *in, int h, int w, int C, float *out, int H, int W,
                               int float16, aoc_stream_t stream);
/* Bilinear (align_corners=True) resize of planes [P,h,w]; plane p = (po, pi) = (p / inner_count,
 * p % inner_count); element (p,y,x) is written at
 *   out[po*out_outer_stride + pi*out_plane_stride + (y*W + x)*out_pixel_stride]
 * so one call can drop [O, F, h, w] results into their channel slice of the [O, 24, H, W] proto-mask
 * buffer or into the reference's [1, H, W, O, F] layout (AEM:604-607, 1054-1058).  An identity-size
 * resize is an exact copy. */
int aoc_resize_bilinear_planes(const float *in, int P, int h, int w, float *out, int H, int W,
                               int inner_count, int64_t out_outer_stride, int64_t out_plane_stride,
                               int64_t out_pixel_stride, aoc_stream_t stream);
/* Atrous sub-sampling of a channel-last map (AEM:533-579, the atrous_obj_pixel_num == 0 branch: pad to a multiple of the rate, view as
 * [h', rate, w', rate, X], keep [:, 0, :, 0]): out [h', w', X] = in[rate * y', rate * x', :] with h' = ceil(h / rate), w' = ceil(w / rate) -- the
 * padding is never selected.  For the embeddings AND the label maps of a pool frame (a device-side gather: no host-side pad / view arithmetic). */
/* Alignment ("Pointer alignment" above): class 16: in, out; every other pointer class 4. */
int aoc_atrous_subsample(const float *in, int h, int w, int X, int rate, float *out, aoc_stream_t stream);
/* torch 'nearest' resize of per-pixel label bits [h,w] -> [H,W]  (AEM:1017-1018). */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_resize_nearest_bits(const uint32_t *in, int h, int w, uint32_t *out, int H, int W,
                            aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-time local matching (csrc/local_grad.hip): what autograd needs of local_matching / local_matching_proxy (AEM:968-1060 over
 * AEM:921-963, the parallel path).  fp32 only.  The reference keeps the unfolded previous frame [HW, C, (2R+1)^2] and the masked distance
 * volume for its backward; here the forward reports the winning previous-frame pixel beside each minimum and the backward needs only
 * that, the saved output and the two maps.
 *
 * aoc_local_window_match_argmin: arguments, limits and `out` of aoc_local_window_match_ex(float16 = 0) (for C = 100 / 128 bit for bit: the
 * register-operand kernel's arithmetic term by term).  arg [n_obj, n_radii, H, W] (out's channel order): the previous-frame pixel
 * cy * W + cx that holds the minimum of that channel's window; ties go to the lowest pixel index (row-major window order, the first
 * occurrence) in every nested window alike; -1 where the value is the padding (no right pixel in the window): out is then exactly 1.0f
 * with transform != 0 and the gradient is zero. */
/* Alignment ("Pointer alignment" above): class 16: query, prev; every other pointer class 4. */
int aoc_local_window_match_argmin(const float *query, const float *prev, const uint32_t *right_bits, int H, int W, int C,
                                  const int32_t *radii_host, int n_radii, const float *obj_bias, int n_obj,
                                  float *out, int32_t *arg, int transform, int atrous_rate, aoc_stream_t stream);

/* Backward of out = T = 2 sigmoid(d + bias[o]) - 1 with d = |q_i - p_arg|^2.  grad_out, T, arg: [n_obj, n_radii, H, W] contiguous;
 * query, prev [H, W, C]; window = the largest window's half-size in pixels (atrous_rate * (radii[last] / atrous_rate)): an arg further
 * than that from its query pixel (Chebyshev) or outside the map counts as -1.  With g = (grad_out * 0.5f) * (1 - T * T):
 *   grad_query [H * W, C]  row i = sum over (o, ch), ascending, of (2 g) * (q_i - p_arg)
 *   grad_prev  [H * W, C]  row j = sum over the (i, o, ch) with arg == j, ascending i, then o, then ch, of (2 g) * (p_j - q_i); every row is
 *                          written, zeros where nobody chose it.  A gather over the query pixels within `window` of j: no atomics.
 *   grad_bias  [n_obj]     sum over the pixels, ascending, of the sum over ch, ascending, of g
 * Pairs with arg < 0 contribute nothing.  Each output may be NULL (nothing is computed for it).  No float atomics, every sum runs in an
 * order fixed by the source: the same buffers give the same bits.  C <= AOC_MAX_CHANNELS, n_radii <= 8, n_obj <= AOC_MAX_OBJECTS,
 * 0 <= window <= 31. */
size_t aoc_local_match_grad_workspace_bytes(int H, int W, int C, int n_radii, int n_obj);
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_local_match_grad(const float *grad_out, const float *T, const int32_t *arg,
                         const float *query, const float *prev, int H, int W, int C, int n_radii, int n_obj, int window,
                         float *grad_query, float *grad_prev, float *grad_bias,
                         void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-time cluster matching (csrc/cluster_grad.hip): what autograd needs of global_matching_cluster2 (AEM:405-478 over AEM:231-332;
 * matching.py:1324-1404 over 506-640).  Set 0 of an object, the k-means code book, is a constant (torch.from_numpy, AEM:279); set 1,
 * centroid_avg (AEM:280), is a differentiable mean of reference rows.  Labels, the assignment and the drawn rows carry no gradient.
 *
 * aoc_proxy_set_match_argmin: aoc_proxy_corr_min (AEM:92-110, 316-319; same arguments, sets as HOST arrays, transform 0 or 1) plus arg,
 * int32, addressed like out: arg[i*out_pixel_stride + set_out_offset[s]] = the slot WITHIN the set (0 .. set_size[s] - 1) of the minimum;
 * ties go to the lowest slot (torch.min's choice on a tie is one of them); -1 where the set is empty or all-ignored (+inf norms): the
 * value is then AOC_PAD_DISTANCE and T exactly 1.0f.  out holds bit for bit what aoc_proxy_corr_min writes for the same arguments (the
 * same fp32 MFMA sequence and the same norm sums; a slot index rides beside each minimum).  C as aoc_proxy_corr_min (a multiple of 4,
 * 4 .. AOC_MAX_CHANNELS), set sizes 0 .. AOC_MAX_CLUSTERS (beyond: AOC_ERR_UNSUPPORTED), any number of sets (a frame has
 * 2 * levels * objects of them; 64 go into one launch).  No workspace.  proxy_sqnorm = NULL is the slow form: every lane sums |p|^2 over
 * all C again for every tile of 16 query pixels. */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_proxy_set_match_argmin(const float *query, int64_t m, int C,
                               const float *proxies, const float *proxy_sqnorm, int n_proxy,
                               int n_set, const int32_t *set_begin_host, const int32_t *set_size_host,
                               const int64_t *set_out_offset_host, const float *set_bias,
                               float *out, int32_t *arg, int64_t out_pixel_stride, int transform, aoc_stream_t stream);

/* The backward of the min over sets (AEM:109 / 319) followed by the proto-mask transform (AEM:467-468).  grad_out, T (the saved
 * transformed output) and arg are addressed as in the forward ([i*pixel_stride + set_out_offset[s]]); query [m, C]; proxies [n_proxy, C];
 * set_bias_index [n_set], HOST: the element of grad_bias the set's bias came from (its object).  With g = (grad_out * 0.5f) * (1 - T*T) and
 * p* = proxies[set_begin[s] + arg] of (pixel i, set s):
 *   grad_query   [m, C]       row i = sum over the sets, ascending, of (2 g) * (q_i - p*)
 *   grad_proxies [n_proxy, C] row r = 2 (p_r * sum g - sum g q_i) over the pairs that chose r; EVERY row is written, with zeros where nobody
 *                             chose it or it lies outside every set
 *   grad_bias    [n_bias]     sum of g over the pixels and over the sets that name that element
 * Pairs with arg < 0 (or >= set_size) contribute nothing.  Each output may be NULL (nothing is computed for it).  Few rows, every one of
 * them hot: the pixels are cut into n_chunk = min(128, ceil(m / 32)) contiguous chunks; a workgroup adds g q_i of one (chunk, set, 32 slots)
 * in pixel order into LDS rows, one thread per channel; a second pass adds the chunks in ascending (set, chunk) order per proxy row.  No
 * float atomics, every sum in an order fixed by (m, sets) alone: the same buffers give the same bits.
 * workspace: align256(n_slot * n_chunk * (C + 1) * 4 + 16) + align256(n_slot * 4 + 16) bytes, n_slot = the sum of the set sizes: bounded
 * in m (at most 128 chunks), it never holds a [m, n_proxy, C] term.  Only needed when grad_proxies or grad_bias is wanted.
 * C and set sizes as the forward; set_bias_index may be NULL when grad_bias is. */
size_t aoc_proxy_set_match_grad_workspace_bytes(int64_t m, int C, int64_t n_slot);
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_proxy_set_match_grad(const float *grad_out, const float *T, const int32_t *arg, int64_t pixel_stride,
                             const float *query, int64_t m, int C, const float *proxies, int n_proxy,
                             int n_set, const int32_t *set_begin_host, const int32_t *set_size_host,
                             const int64_t *set_out_offset_host, const int32_t *set_bias_index_host, int n_bias,
                             float *grad_query, float *grad_proxies, float *grad_bias,
                             void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The backward of aoc_build_proxies' set 1 (AEM:280, centroid_avg: cluster j of segment s is the mean of the rows fg[p] of the GLOBAL
 * kept-row array over the segment-local p with label == j; the reference's indexing, reproduced as is).  grad_proxies
 * [n_seg, 2, kmax, C] (only [:, 1] is read); fg_rows, n_fg (device), seg_offsets [n_seg + 1], seg_k [n_seg] and the packed labels
 * [rows_capacity] as aoc_build_proxies takes them.  grad_pool [pool_rows, C]:
 *   row fg_rows[p] = sum over the segments s with length > p, ascending, of grad_proxies[s, 1, labels_s[p]] / count_s(labels_s[p]),
 * count_s(j) = the number of p in segment s with label j (what the mean was divided by); every other row is zero.  A gather, one wave per
 * kept position: a row shared by several segments needs neither atomics nor ordering.  Multi-level segment lists
 * (n_seg = levels * objects, aoc_kmeans_replicate_levels) are segments like any other.  workspace: the counts, [n_seg, kmax] int32. */
size_t aoc_centroid_avg_grad_workspace_bytes(int n_seg, int kmax);
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_centroid_avg_grad(const float *grad_proxies, int C, const int32_t *fg_rows, const int32_t *n_fg,
                          const int32_t *seg_offsets, const int32_t *seg_k, const int32_t *labels,
                          int n_seg, int kmax, int64_t rows_capacity, float *grad_pool, int64_t pool_rows,
                          void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-time front end of the proto-mask tensor (csrc/frontend_grad.hip; aoc_amd.frontend_train): streaming kernels, lanes along hw.
 * A thread moves 16 bytes (four consecutive pixels) when every row it touches starts on a 16-byte boundary -- hw (inner) and every stride
 * a multiple of 4 floats, every pointer 16-byte aligned; otherwise the same kernel runs with one pixel per thread and 4-byte accesses,
 * still coalesced.  The choice depends on shapes and pointers alone and changes no bit.  No float atomics; every sum in ascending object
 * order; every argmin takes the lowest (object, channel) among equal minima, the order of the reference's concatenation (AEM:13-19).
 *
 * The backward of aoc_masked_mean_pool for one frame (ATT:134-153; ATT:81-87 / 136-142 are the forward lines it differentiates):
 *   Np_o = sum_p l[o,p],  Nn_o = sum_p (1 - l[o,p])       (computed here: per object, thread t of 256 adds pixels t, t + 256, ... in
 *                                                          ascending order, then a binary tree over the 256 partial sums)
 *   grad_emb[c,p] = sum_o ( grad_pos[o,c] / (Np_o + eps) * l[o,p]  +  grad_neg[o,c] / (Nn_o + eps) * (1 - l[o,p]) )
 * added in ascending o, an object's positive term before its negative one.  labels [n_obj, hw], or [hw, n_obj] when labels_pixel_major
 * (read with 4-byte accesses at a stride of n_obj floats between lanes then: not coalesced, the one operand here that is not); grad_pos, grad_neg [n_obj, C] (grad_neg may be NULL: its term is left out); grad_emb [C, hw], the
 * planes of the caller's [C, h, w] embedding -- the channel-last copy the forward reads is not differentiated through.  Labels get no
 * gradient.  n_obj <= 32.  workspace: the 2 n_obj counts. */
size_t aoc_masked_mean_pool_grad_workspace_bytes(int n_obj);
int aoc_masked_mean_pool_grad(const float *grad_pos, const float *grad_neg, const float *labels, int64_t hw, int C, int n_obj, int labels_pixel_major,
                              float epsilon, float *grad_emb, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The backward of aoc_fg2bg_min (AEM:9-23; torch.min of AEM:20 sends the gradient to one entry): per x the lowest entry (o1, c1) of
 * dis [n_obj, n_ch, inner] and the lowest entry (o2, c2) among the objects other than o1 are recomputed from the saved dis (no index
 * tensor); winner(o, x) = (o1, c1) for o != o1 and (o2, c2) for o = o1, so
 *   grad_dis[o1, c1, x] = sum over o != o1, ascending from 0.0f, of grad_out[o, x];   grad_dis[o2, c2, x] = grad_out[o1, x];   0 elsewhere.
 * dis / grad_dis / grad_out are addressed with their object strides as in the forward; all n_obj * n_ch * inner elements of grad_dis are
 * written.  n_obj >= 2 (one object is the identity, AEM:10-11). */
int aoc_fg2bg_grad(const float *grad_out, int64_t grad_out_obj_stride, const float *dis, int n_obj, int n_ch, int64_t inner, int64_t dis_obj_stride,
                   float *grad_dis, int64_t grad_dis_obj_stride, aoc_stream_t stream);

/* The training form of aoc_proto_finish plus the concatenation of aocnet.py:341-358, one launch each way.  The five matching outputs as
 * planes: global_fg, proxy_fg [n_obj, 1, hw]; cluster_fg [n_obj, n_cluster, hw]; local_fg, local_proxy_fg [n_obj, n_local, hw];
 * prev_label [n_obj, hw] (aocnet.py:155).  feat [n_obj, n_ch, hw], channels in the order of aocnet.py:355-358:
 *   global | cluster | proxy | local | local proxy | previous mask | (background != 0: local background [n_local] | global background)
 * background channel = per channel the min over the OTHER objects (aocnet.py:349-353; the values of aoc_fg2bg_min bit for bit); one
 * object copies its foreground (AEM:10-11).  n_ch = aoc_proto_aggregate_channels.  Each source is read once.
 * The backward reads grad_feat and the saved feat (the foreground channels in it name the winners: lowest object among equal minima):
 *   grad_fg[o'] = grad_feat_fg[o'], then + grad_feat_bg[o] for every o with winner(o) = o', in ascending o;
 * one object adds the two.  The mask channel gets none.  A NULL gradient pointer skips that source. */
int aoc_proto_aggregate_channels(int n_cluster, int n_local, int background);
int aoc_proto_aggregate(const float *global_fg, const float *cluster_fg, const float *proxy_fg, const float *local_fg, const float *local_proxy_fg,
                        const float *prev_label, int n_obj, int64_t hw, int n_cluster, int n_local, int background, float *feat, aoc_stream_t stream);
int aoc_proto_aggregate_grad(const float *grad_feat, const float *feat, int n_obj, int64_t hw, int n_cluster, int n_local, int background,
                             float *grad_global, float *grad_cluster, float *grad_proxy, float *grad_local, float *grad_local_proxy,
                             aoc_stream_t stream);

/*
 * Training-time calibration gates (csrc/gate_grad.hip; aoc_amd.gates_train): the backward of IA_gate, GCT and the conditioning block.
 * fp32.  No float atomics; every sum runs in an order fixed by the shapes and the pointers' 16-byte alignment, so the same buffers give
 * the same bits.  The three streaming entries (channel_scale_grad, gct_scale_grad, cond_scale_grad) cut a plane by the alignment of the
 * plane they write (of grad_y for the plane dot): up to 3 scalar floats in front, 16 bytes per lane for the body, up to 3 scalars behind;
 * sources are loaded 16 bytes per lane at 4-byte alignment, so source planes may sit at other misalignments.  Every pointer marked
 * optional may be NULL and its work is skipped.  N, n_obj <= AOC_MAX_OBJECTS.  The three streaming entries take up to 2^31 - 1 planes
 * (one workgroup row per plane on the grid's x axis); aoc_film_gain_grad wants n_obj + channels <= 65 535 and aoc_cond_codes_grad
 * N + 2 C + D <= 65 535 (their rows ride on the grid's y axis); beyond that they return AOC_ERR_UNSUPPORTED and enqueue nothing.
 *
 * The backward of y[p,:] = gain[p] * x[p,:] (ATT:16 `a * x`, gct.py:36 `x * gate`, CLB:84), one pass over the two inputs:
 *   grad_x[p,i] = gain[p] * grad_y[p,i]               (optional; needs gain)
 *   dgain[p]    = sum_i grad_y[p,i] * x[p,i]           (optional; needs x)
 * One workgroup of T threads per plane (T = 256 up to 2 048 float4 per plane, else 1 024).  Order of the sum: thread t adds its front
 * scalar, the float4 t, t + T, ... (x, y, z, w in turn) and its back scalar, every product rounded first; the 64 lanes of a wave by xor
 * butterfly (32, 16, ... 1); the waves in ascending order from 0.0f.  With grad_x == NULL this is the plane dot of the other backwards. */
int aoc_channel_scale_grad(const float *grad_y, const float *x, const float *gain, int64_t planes, int64_t hw, float *grad_x, float *dgain,
                           aoc_stream_t stream);

/* Through gain = 1 + tanh(head W^T + b) (ATT:12-15; the last linear of CLB:81-82):  da[o,c] = dgain[o,c] * (1 - t^2), t = gain[o,c] - 1;
 *   grad_head[o,d]   = sum_c da[o,c] * weight[c,d]     ascending c from 0.0f
 *   grad_weight[c,d] = sum_o da[o,c] * head[o,d]       ascending o from 0.0f
 *   grad_bias[c]     = sum_o da[o,c]                   ascending o from 0.0f
 * each optional.  dgain, gain [n_obj, channels]; head [n_obj, head_dim]; weight [channels, head_dim]. */
int aoc_film_gain_grad(const float *dgain, const float *gain, const float *head, const float *weight, int n_obj, int head_dim, int channels,
                       float *grad_head, float *grad_weight, float *grad_bias, aoc_stream_t stream);

/* The backward of aoc_gct_gate (gct.py:19-34): dgate, gate, plane_sums [N, C]; du = dgate * (1 - t^2), t = gate - 1.
 *   l2 (gct.py:20-21): e_c = sqrt(S_c + eps) alpha_c, M = mean_c e_c^2, r = sqrt(M + eps), dM = -1/2 (sum_c du_c e_c gamma_c) / (r (M + eps)),
 *        de_c = du_c gamma_c / r + 2 e_c dM / C,      dsum[n,c] = de_c alpha_c / (2 sqrt(S_c + eps)),  grad_alpha_c += de_c sqrt(S_c + eps)
 *   l1 (gct.py:28-29): e_c = S_c alpha_c, M = mean_c |e_c|, r = M + eps, dM = -(sum_c du_c e_c gamma_c) / r^2,
 *        de_c = du_c gamma_c / r + sign(e_c) dM / C,  dsum[n,c] = de_c alpha_c,                        grad_alpha_c += de_c S_c
 *        (sign(0) = 0, torch's choice for d|e|)
 *   both: grad_gamma_c += du_c e_c / r,  grad_beta_c += du_c.
 * The sums over c: thread t of 256 adds c = t, t + 256, ..., then the wave butterfly, then the wave sums as (0 + 1) + (2 + 3).  The sums
 * over n: ascending n from 0.0f.  `beta` is not read (the saved gate carries it).  dsum and the three gradients [C] are optional. */
int aoc_gct_gate_grad(const float *dgate, const float *gate, const float *plane_sums, const float *alpha, const float *gamma, const float *beta, int N,
                      int C, float eps, int l1_mode, float *dsum, float *grad_alpha, float *grad_gamma, float *grad_beta, aoc_stream_t stream);

/* GCT's apply pass (gct.py:19-36): grad_x[p,i] = grad_y[p,i] * gate[p] + dsum[p] * f'(x[p,i]), f' = 1 / 2x / sign(x) for aoc_plane_reduce's
 * mode 0 / 1 / 2.  No sum. */
int aoc_gct_scale_grad(const float *grad_y, const float *x, const float *gate, const float *dsum, int mode, int64_t planes, int64_t hw, float *grad_x,
                       aoc_stream_t stream);

/* The backward of aoc_cond_codes (CLB:68-80).  dcode [N, 2C + D] = (dcode_1 | dcode_2 | dcode_3); gap, plane_means [N, C]; head [N, D];
 * w1, w2 [C, C]; w3 [D, D].  Each output optional:
 *   dgap[n,j]      = sum_i dcode_1[n,i] w1[i,j]                       grad_head[n,j] = sum_i dcode_3[n,i] w3[i,j]          ascending i
 *   dpx[n,j]       = (sum_m dd[m,j]) - dd[n,j],  dd[m,j] = sum_i dcode_2[m,i] w2[i,j]     (CLB:69 backwards; ascending m, ascending i)
 *   grad_w1[i,j]   = sum_n dcode_1[n,i] gap[n,j]     grad_w3[i,j] = sum_n dcode_3[n,i] head[n,j]     grad_b*[i] = sum_n dcode_*[n,i]
 *   grad_w2[i,j]   = sum_n dcode_2[n,i] delta[n,j],  delta[n,j] = (sum_m plane_means[m,j]) - plane_means[n,j] as aoc_cond_codes forms it
 * all sums ascending from 0.0f.  C may be 0: the third code alone is the backward of one square aoc_linear (conditioning_layer's
 * mlp_layer, CLB:46). */
int aoc_cond_codes_grad(const float *dcode, const float *gap, const float *plane_means, const float *head, const float *w1, const float *w2,
                        const float *w3, int N, int C, int D, float *dgap, float *dpx, float *grad_head, float *grad_w1, float *grad_b1, float *grad_w2,
                        float *grad_b2, float *grad_w3, float *grad_b3, aoc_stream_t stream);

/* The conditioning block's apply pass (CLB:68, 72, 84 with CLB:36-43):
 *   grad_x[n,c,p] = (grad_y[n,c,p] * gain[n,c] + (scores[n,p] > threshold[n] ? dgap[n,c] / hw : 0)) + dpx[n,c] / hw
 * The mask is recomputed from the scores and threshold aoc_cond_gate_pool_ex emitted, with the same strict `>`; no mask tensor exists.
 * dgap, dpx optional (their term is 0.0f); grad_y optional together with gain (the first term is dropped: conditioning_layer's own
 * backward, CLB:36-43, with dpx == NULL).  phi_layer gets no gradient: CLB:36 compares. */
int aoc_cond_scale_grad(const float *grad_y, const float *gain, const float *scores, const float *threshold, const float *dgap, const float *dpx, int N,
                        int C, int64_t hw, float *grad_x, aoc_stream_t stream);

/*
 * Training-time decoder forms (csrc/norm_grad.hip; aoc_amd.decoder_train): the backward of the Bottleneck's normalisations and of the
 * modulators' concatenation gate.  fp32, no float atomics, every sum in an order fixed by the shapes and the pointers' 16-byte alignment;
 * every pointer marked optional may be NULL and its work is skipped; every argument is validated before the first launch, and a call that
 * is rejected enqueues nothing.  N, n_obj <= AOC_MAX_OBJECTS; the planes ride on the grid's x axis, so N * C (n_obj * (Cx + Cm)) may reach
 * 2^31 - 1 -- the forward's 65 535 limit is not inherited; beyond that AOC_ERR_UNSUPPORTED.
 *
 * The backward of aoc_groupnorm_relu and of aoc_groupnorm_relu_scale (gct.py:71-72, 75-76, 79-90 `out = self.bn3(out); out += residual;
 * out = self.relu(out)`, and ATT:16 `a * x` of the gate behind it, decoding_module.py:196,198 / :206,208):
 *   y = [gain[n,c] *] [relu]( z ),   z = xhat * gamma[c] + beta[c] [+ residual],   xhat = (x - mean) * rstd.
 * grad_y, x, residual (optional) [N, C, hw]; stats [N * groups][2] = (mean, rstd) as the forward left them at the start of its workspace;
 * gamma, beta [C] or NULL (1, 0); gain [N, C] or NULL (the ungated form).  With a = relu(z) (z when relu == 0), da = gain * grad_y (grad_y
 * without gain), dz = da where z > 0 else 0 (da when relu == 0; the strict `>` of torch's ReLU backward), M = (C / groups) * hw:
 *   A[n,c] = sum_p dz        B[n,c] = sum_p dz * xhat        dgain[n,c] = sum_p grad_y * a                          (plane sums)
 *   s1[n,g] = sum_{c in g} gamma_c * A[n,c]        s2[n,g] = sum_{c in g} gamma_c * B[n,c]                           (ascending c from 0.0f)
 *   grad_gamma[c] = sum_n B[n,c]                   grad_beta[c] = sum_n A[n,c]                                      (ascending n from 0.0f)
 *   grad_residual = dz                             grad_x = rstd * ((gamma_c * dz - s1 / M) - xhat * (s2 / M)),     M as (float)M
 * grad_x, grad_residual [N, C, hw], grad_gamma, grad_beta [C] and dgain [N, C] are each optional, and each has the same bits whether it is
 * asked for alone or with the others.  z is recomputed with the forward's own float expression (x * a + b, a = rstd * gamma_c,
 * b = beta_c - mean * a, then + residual), so the mask is the forward's.  Plane sums: one workgroup of T threads per plane (T = 256 up to
 * 2 048 float4 per plane, else 1 024), the plane cut by grad_y's alignment, in aoc_channel_scale_grad's order: thread t adds its front scalar,
 * the float4 t, t + T, ... (x, y, z, w in turn) and its back scalar, every product rounded first; the 64 lanes of a wave by xor butterfly
 * (32, 16, ... 1); the waves in ascending order from 0.0f.  Three launches (plane pass, the small sums, apply pass): grad_y, x and the residual
 * are read at most twice, every gradient is written once, nothing of activation size is stored in between.  The apply pass cuts a plane by
 * the alignment of grad_x's plane (grad_residual's when grad_x == NULL).  The workspace holds A, B [N, C] and (s1, s2) / M [N * groups][2]; it
 * is needed when grad_x, grad_gamma or grad_beta is asked for (else it may be NULL): AOC_ERR_WORKSPACE when it is short. */
size_t aoc_groupnorm_relu_grad_workspace_bytes(int N, int C, int groups);
int aoc_groupnorm_relu_grad(const float *grad_y, const float *x, const float *residual, const float *stats, const float *gamma, const float *beta,
                            const float *gain, int N, int C, int64_t hw, int groups, int relu, float *grad_x, float *grad_residual, float *grad_gamma,
                            float *grad_beta, float *dgain, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The backward of aoc_cat_film_scale (decoding_module.py:193-194 / :203-204: `torch.cat([x, x_memory], dim=1)` and the IA_gate's `a * x`,
 * ATT:16) in one pass; the concatenation is never materialised.  grad_y [n_obj, Cx + Cm, hw]; x [n_obj, Cx, hw]; mem [n_obj, Cm, hw] (may
 * alias x; NULL with Cm = 0); gain [n_obj, Cx + Cm].  Each output optional:
 *   grad_x[o, c]   = gain[o, c] * grad_y[o, c]              (c < Cx; needs gain)
 *   grad_mem[o, c] = gain[o, Cx + c] * grad_y[o, Cx + c]    (needs gain and Cm >= 1; the modulators' memory is detached and asks for none)
 *   dgain[o, c]    = sum_p grad_y[o, c, p] * cat(x, mem)[o, c, p]            (needs x, and mem when Cm >= 1)
 * One workgroup per plane of grad_y, the plane cut by GRAD_Y's alignment whatever is written (so dgain's bits do not depend on the other
 * outputs), the sum in aoc_channel_scale_grad's order (above); gradient planes at another misalignment are stored 16 bytes per lane at 4-byte
 * alignment.  dgain then goes through aoc_film_gain_grad to grad_head, grad_weight and grad_bias. */
int aoc_cat_film_scale_grad(const float *grad_y, const float *x, const float *mem, const float *gain, int n_obj, int Cx, int Cm, int64_t hw, float *grad_x,
                            float *grad_mem, float *dgain, aoc_stream_t stream);

/*
 * Training-time decoder tail (csrc/tail_grad.hip; aoc_amd.tail_train): the backward of aoc_shortcut_stage_enqueue, the apply pass of a delta
 * gate, the prediction head with the index of its background minimum, and their gradients.  fp32, no float atomics, every sum in an order
 * fixed by the shapes and the pointers' 16-byte alignment; every pointer marked optional may be NULL and its work is skipped, and each
 * optional output has the same bits alone as with the others; every argument is validated before the first launch, and a call that is
 * rejected enqueues nothing.  N <= AOC_MAX_OBJECTS; planes ride on the grid's x axis (N * C up to 2^31 - 1).
 *
 * The shortcut stage, out = gain * cat(bicubic(x), low) with gain = 1 + tanh(W [IA_head | delta(px)] + b), px = the plane means of the
 * concatenation, delta(px)[n] = sum_m px[m] - px[n] (decoding_module.py:163, 170-176).  grad_out [N, Ce + Cr, H, W]; x [N, Ce, h, w];
 * low [N, Cr, H, W] (NULL with Cr = 0).
 *
 * aoc_shortcut_stage_grad_dots (pass A):
 *   t[n, c] = U^T grad_out[n, c] [h, w]   the adjoint of the bicubic upsample alone, with aoc_bicubic_cat_scale's own weights (the integer
 *       coordinate split, A = -0.75, clamped taps), in gather form: u[I, j] = sum over the output columns J in ascending order, the taps
 *       k = 0..3 of each in turn, of wx[J][k] * grad_out[I, J] where clamp(ix(J) + k - 1) == j; then t[i, j] = the same over the output rows
 *       I with wy and u.  Each product is rounded, then added, from 0.0f.  Clamped taps that land on one border pixel are all added; a
 *       coarse pixel no tap reaches is 0.0f.  Written to t_out [N, Ce, h, w], or kept in the workspace when t_out == NULL.
 *   dgain[n, c < Ce] = sum_ij x * t (= <grad_out, bicubic(x)>): grad_out is read once (plus the fine rows two neighbouring bands share) and
 *       the upsample is never formed.  A workgroup owns a band of coarse rows: thread t of 256 adds x[f] * t[f] for the band's elements
 *       f = t, t + 256, ... (row-major), the xor butterfly over a wave, the four wave sums in ascending order; then the bands in ascending
 *       order from 0.0f.  The band height follows from (N * Ce, h, w, H, W) alone.
 *   dgain[n, Ce + c] = the plane dot of grad_out[n, Ce + c] and low[n, c]: aoc_channel_scale_grad itself, called per object.
 * dgain [N, Ce + Cr] is optional (needs x, and low when Cr >= 1).  The workspace is needed unless t_out is given and dgain is not.
 *
 * aoc_shortcut_stage_grad_apply (pass B), after aoc_film_gain_grad and the delta pull-back dpx[n] = sum_m dd[m] - dd[n] on [N, Ce + Cr]:
 *   grad_x[n, c, i, j] = gain[n, c] * t + (cy[i] * cx[j]) * (dpx[n, c] / (float)(H W))     in place over t (grad_x holds t on entry)
 *   grad_low[n, c, p]  = gain[n, Ce + c] * grad_out[n, Ce + c, p] + dpx[n, Ce + c] / (float)(H W)
 * cy, cx = the column sums of the two 1-D interpolation matrices, formed as aoc_bicubic_plane_mean forms them.  gain == NULL is 1 and
 * dpx == NULL is 0 (with both, a plain resize adjoint: grad_x is t).  grad_x and grad_low (needs Cr >= 1) are optional.  grad_low's planes are
 * cut by their own alignment: up to three scalars in front, 16 bytes per lane, up to three scalars behind. */
size_t aoc_shortcut_stage_grad_workspace_bytes(int N, int Ce, int h, int w, int H, int W);
int aoc_shortcut_stage_grad_dots(const float *grad_out, const float *x, const float *low, int N, int Ce, int Cr, int h, int w, int H, int W, float *t_out,
                                 float *dgain, void *workspace, size_t workspace_bytes, aoc_stream_t stream);
int aoc_shortcut_stage_grad_apply(const float *grad_out, const float *gain, const float *dpx, int N, int Ce, int Cr, int h, int w, int H, int W, float *grad_x,
                                  float *grad_low, aoc_stream_t stream);

/* The apply pass of a delta gate, y = gain * x with gain = 1 + tanh(W [IA_head | delta(plane means of x)] + b) (decoding_module.py:126-130,
 * :181-185), after aoc_channel_scale_grad (dgain), aoc_film_gain_grad and the delta pull-back:
 *   grad_x[n, c, p] = gain[n, c] * grad_y[n, c, p] + dpx[n, c] / (float)hw        (dpx == NULL: no shift)
 * 16 bytes per lane, the plane cut by grad_x's alignment; grad_y is read at 4-byte alignment. */
int aoc_delta_gate_grad_apply(const float *grad_y, const float *gain, const float *dpx, int N, int C, int64_t hw, float *grad_x, aoc_stream_t stream);

/* aoc_logit_head that also writes arg [hw] (int32): the object n >= 1 whose bg logit is the minimum.  The strict `<` of aoc_logit_head: the
 * lowest n wins a tie, a NaN is never selected, and 0 stands for "no object" (every bg logit NaN or +inf).  With N = 1 arg is untouched (and
 * may be NULL).  The channel sums are repeated term by term: pred is bit-equal to aoc_logit_head's. */
int aoc_logit_head_argmin(const float *x, const float *wb_fg, const float *wb_bg, int64_t stride, int N, int C, int64_t hw, float *pred, int32_t *arg,
                          aoc_stream_t stream);
/* Its backward.  g = grad_pred [N, hw]; x [N, C, hw] (always needed: its planes' alignment cuts the sums); wfg, wbg = the first C columns of
 * the rows of wb_fg, wb_bg.  Each output optional:
 *   grad_x[n, c, p]     = g[n, p] * wfg[n, c] + (n == arg[p] ? g[0, p] * wbg[n, c] : 0)             (needs wb_fg, and wb_bg when N > 1)
 *   grad_wb_fg[n, c]    = sum_p g[n, p] * x[n, c, p]                 grad_wb_fg[n, C] = sum_p g[n, p]
 *   grad_wb_bg[n, c]    = sum_{p: arg[p] == n} g[0, p] * x[n, c, p]  grad_wb_bg[n, C] = sum_{p: arg[p] == n} g[0, p]     (n >= 1; row 0 is 0)
 * grad_wb_* [N, C + 1] contiguous.  One workgroup per column (n, c): x is read once, grad_x written once.  The sums run in
 * aoc_channel_scale_grad's order with the plane cut by x's alignment (by grad_pred[n]'s for the bias column) whatever is written; the pixels
 * of other objects add +0.0f to a bg sum. */
int aoc_logit_head_grad(const float *grad_pred, const int32_t *arg, const float *x, const float *wb_fg, const float *wb_bg, int64_t stride, int N, int C,
                        int64_t hw, float *grad_x, float *grad_wb_fg, float *grad_wb_bg, aoc_stream_t stream);
/* aoc_background_merge with the same arg [hw], and its backward: grad_fg = grad_pred; grad_bg[n, p] = (n == arg[p]) * grad_pred[0, p], row 0
 * zero.  Both gradients optional. */
int aoc_background_merge_argmin(const float *fg, const float *bg, int N, int64_t hw, float *pred, int32_t *arg, aoc_stream_t stream);
int aoc_background_merge_grad(const float *grad_pred, const int32_t *arg, int N, int64_t hw, float *grad_fg, float *grad_bg, aoc_stream_t stream);

/*
 * Training-time ASPP (csrc/aspp_grad.hip; aoc_amd.aspp_train): the backward of aoc_plane_sum_sumsq / aoc_gct_gate_multi /
 * aoc_channel_scale_multi (aspp.py:19 four times, :46) and of aoc_groupnorm_cat_relu with the GCT behind it (aspp.py:21-23 four times,
 * :61-65).  fp32, no float atomics, every sum in an order fixed by the shapes and the pointers' 16-byte alignment; every pointer marked
 * optional may be NULL and its work is skipped, and each optional output has the same bits alone as with the others; every argument is
 * validated before the first launch (outputs that overlap an input or each other: AOC_ERR_INVALID_ARG), and a call that is rejected enqueues
 * nothing.  N <= AOC_MAX_OBJECTS; planes ride on the grid's x axis (up to 2^31 - 1); pointer lists are host arrays of 1 .. 8 device
 * pointers (other counts: AOC_ERR_INVALID_ARG), as aoc_channel_scale_multi's.
 *
 * The front, v_k = x * gate_k(plane sums of x^2) for k < n_set and mean = sum x / hw:
 *
 * aoc_plane_dot_multi: dots[k, p] = sum_i g_k[p, i] * x[p, i] for the n_set gradient tensors g_k [planes, hw]; dots [n_set, planes].  Set k's
 * plane is cut by g_k's own alignment and summed in aoc_channel_scale_grad's order, so set k is bit-equal to aoc_channel_scale_grad(g_k, x)
 * with grad_x == NULL.  Where the sets share one cut, each 16 bytes of x are loaded once for all of them. */
int aoc_plane_dot_multi(const float *x, const float *const *g_ptrs, int n_set, int64_t planes, int64_t hw, float *dots, aoc_stream_t stream);

/* aoc_gct_gate_grad for n_set parameter sets over ONE [N, C] array of plane sums, one workgroup per set: dgate, gate [n_set, N, C]; alpha,
 * gamma, beta [n_set, C] (beta is not read).  Set k of dsum [n_set, N, C] and of grad_alpha, grad_gamma, grad_beta [n_set, C] carries the
 * bits of aoc_gct_gate_grad with row k; dsum_total [N, C] = sum_k dsum[k] in ascending k from 0.0f.  All five outputs are optional; the
 * workspace is needed (AOC_ERR_WORKSPACE) only for dsum_total without dsum.  Both modes of aoc_gct_gate_grad (l1_mode) are supported. */
size_t aoc_gct_gate_multi_grad_workspace_bytes(int n_set, int N, int C);
int aoc_gct_gate_multi_grad(const float *dgate, const float *gate, const float *plane_sums, const float *alpha, const float *gamma, const float *beta,
                            int n_set, int N, int C, float eps, int l1_mode, float *dsum_total, float *dsum, float *grad_alpha, float *grad_gamma,
                            float *grad_beta, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The apply pass of the front (l2 mode: d(sum x^2)/dx = 2 x):
 *   grad_x[p, i] = ((sum_k g_k[p, i] * gates[k, p]) + (2 * dsum_total[p]) * x[p, i]) + dmean[p] / (float)hw
 * in exactly this order: the sum over k starts from the product of set 0 and adds the sets in ascending k; then the second term; then,
 * unless dmean == NULL, the mean's share.  2 * dsum_total is exact, so with n_set = 1 and dmean == NULL the result is bit-equal to
 * aoc_gct_scale_grad in mode 1.  The plane is cut by grad_x's alignment; g_k and x are read 16 bytes per lane at any misalignment. */
int aoc_channel_scale_multi_grad_apply(const float *const *g_ptrs, const float *gates, const float *x, const float *dsum_total, const float *dmean,
                                       int n_set, int64_t planes, int64_t hw, float *grad_x, aoc_stream_t stream);

/* The back: out = G[n, cc] * cat, cat = aoc_groupnorm_cat_relu(u_0 .. u_{n_src-1}, tail) with relu = 1, G = aoc_gct_gate(plane_sumsq of cat)
 * in l2 mode.  grad_out [N, C_total, hw], C_total = n_src * C_src + C_tail; u_k [N, C_src, hw]; stats [n_src][N * groups][2] = (mean, rstd) as
 * aoc_groupnorm_cat_relu leaves them at the start of its workspace; gamma, beta [n_src, C_src] or NULL (1, 0); tail [N, C_tail] (before its
 * ReLU; NULL with C_tail = 0); plane_sumsq, gate [N, C_total]; gct_alpha, gct_gamma [C_total].  With z = u * a + b (a = rstd * gamma,
 * b = beta - mean * a: the forward's own float expression), m = (z > 0), cat = max(z, 0), xhat = (u - mean) * rstd, M = (C_src / groups) * hw:
 *   plane pass   P1 = sum g * cat   P2 = sum m ? g : 0   P3 = sum m ? g * xhat : 0   P4 = sum cat   P5 = sum cat * xhat     (source planes)
 *                Sg = sum g,  P1 = relu(tail) * Sg                                                                           (tail planes)
 *                one workgroup per plane of grad_out, the plane cut by grad_out's alignment, in aoc_channel_scale_grad's order
 *   small        ds, grad_gct_alpha, grad_gct_gamma, grad_gct_beta = aoc_gct_gate_grad's arithmetic with dgate = P1
 *                A = G * P2 + (2 * ds) * P4        B = G * P3 + (2 * ds) * P5
 *                s1[k, n, g] = sum_{c in g} gamma_c * A     s2 likewise with B                                 (ascending c from 0.0f)
 *                grad_gamma[k, c] = sum_n B        grad_beta[k, c] = sum_n A                                   (ascending n from 0.0f)
 *                grad_tail[n, c] = tail > 0 ? G * Sg + ((2 * ds) * (float)hw) * tail : 0
 *   apply pass   dz = m ? g * G + (2 * ds) * cat : 0        grad_u_k = rstd * ((gamma_c * dz - s1 / M) - xhat * (s2 / M)),  M as (float)M
 *                the plane cut by grad_u_k's alignment
 * grad_out and u are read twice, every gradient is written once, nothing of activation size is stored in between.  grad_u_ptrs (NULL, or a
 * list of n_src pointers of which any may be NULL), grad_gamma, grad_beta [n_src, C_src], grad_tail [N, C_tail] and the three GCT gradients
 * [C_total] are each optional.  The workspace (P, ds and (s1, s2) / M) is always needed: AOC_ERR_WORKSPACE when it is short. */
size_t aoc_groupnorm_cat_relu_grad_workspace_bytes(int n_src, int N, int C_src, int C_tail, int groups);
int aoc_groupnorm_cat_relu_grad(const float *grad_out, const float *const *u_ptrs, int n_src, int N, int C_src, int64_t hw, int groups, const float *stats,
                                const float *gamma, const float *beta, const float *tail, int C_tail, const float *plane_sumsq, const float *gate,
                                const float *gct_alpha, const float *gct_gamma, float gct_eps, float *const *grad_u_ptrs, float *grad_gamma,
                                float *grad_beta, float *grad_tail, float *grad_gct_alpha, float *grad_gct_gamma, float *grad_gct_beta, void *workspace,
                                size_t workspace_bytes, aoc_stream_t stream);

/* ---- round 4: fused per-frame launches (each replaces several of the calls above and computes the same expressions term by term, so
 * the outputs equal theirs bit for bit; hotpath.proto_mask_features and aoc_frame_enqueue both use them) ---------------------------- */

/* aoc_resize_bilinear_planes with one more level of output addressing: plane p = (group, outer, inner), groups of
 * outer_count * inner_count planes land out_group_stride apart (the two local-matching results of a frame -> two channel ranges of the
 * proto-mask tensor, aocnet.py:355, in one launch). */
int aoc_resize_bilinear_planes_grouped(const float *in, int P, int h, int w, float *out, int H, int W, int inner_count, int outer_count,
                                       int64_t out_group_stride, int64_t out_outer_stride, int64_t out_plane_stride, int64_t out_pixel_stride,
                                       aoc_stream_t stream);

/* local_matching AND local_matching_proxy (AEM:968-1156 as aocnet.py:255,328 calls them: same query, same label bits, fp32, atrous rate 1)
 * in one launch: out_a from prev_a (the previous frame's embedding), out_b from prev_b (its per-pixel proxy map). */
/* Alignment ("Pointer alignment" above): class 16: query, prev_a, prev_b; every other pointer class 4. */
int aoc_local_window_match_pair(const float *query, const float *prev_a, const float *prev_b, const uint32_t *right_bits, int H, int W, int C,
                                const int32_t *radii_host, int n_radii, const float *obj_bias, int n_obj, float *out_a, float *out_b,
                                int transform, aoc_stream_t stream);

/* The half-resolution operands of both local matchings (AEM:938-941 with MODEL_LOCAL_DOWNSAMPLE) in one launch:
 *   q2, p2 [H2, W2, C]  = aoc_resize_bilinear_hwc of cur_emb / prev_emb [h, w, C]
 *   pm2    [H2, W2, C]  = aoc_resize_bilinear_hwc of aoc_label_mix(prev_labels [h*w, n_obj], prev_pos [n_obj, C])   (aocnet.py:325)
 *   bits2  [H2 * W2]    = aoc_resize_nearest_bits of aoc_label_bits(prev_labels)
 * Optional small tables filled by the same launch (NULL / 0 = off): set_bias_out [n_pair_sets + n_obj] = the per-set bias table of the
 * correlation launch (set s < n_pair_sets belongs to object (s / 2) % n_obj, set n_pair_sets + o to object o); two float copies
 * copy_dst_x[0 .. n_copy_x) = copy_src_x[..] (the pooled reference heads into the k = 1 rows of the proxy table). */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_local_prep(const float *cur_emb, const float *prev_emb, const float *prev_labels, const float *prev_pos, int h, int w, int C, int n_obj,
                   float *q2, float *p2, float *pm2, uint32_t *bits2, int H2, int W2,
                   const float *obj_bias, int n_pair_sets, float *set_bias_out,
                   const float *copy_src_a, float *copy_dst_a, int n_copy_a, const float *copy_src_b, float *copy_dst_b, int n_copy_b,
                   aoc_stream_t stream);

/* The tail of a frame's proto-mask tensor feat [n_obj, n_ch, hw] (object stride obj_stride floats) in one launch, aocnet.py:349-358:
 * channels [ch_local_bg, +n_local) = foreground2background of [ch_local, +n_local), channel ch_global_bg = foreground2background of
 * ch_global, channel ch_prev_mask = prev_labels [hw, n_obj] transposed; head [n_obj, 4 C] = (ref_pos | ref_neg | prev_pos | prev_neg),
 * ATT:188.  A channel index < 0 / head == NULL switches that part off. */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_proto_finish(float *feat, int n_obj, int64_t hw, int64_t obj_stride, int ch_local, int n_local, int ch_local_bg, int ch_global, int ch_global_bg,
                     int ch_prev_mask, const float *prev_labels, const float *ref_pos, const float *ref_neg, const float *prev_pos, const float *prev_neg,
                     int C, float *head, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * foreground2background, AEM:9-23: the reference concatenates the OTHER objects' maps along dim 1
 * and reduces that dim, so  out[o, 0, x] = min over o' != o and over channels c of dis[o', c, x].
 *  dis: object o at dis + o*dis_obj_stride holds [n_ch, inner]; out: object o at out + o*out_obj_stride
 *  holds [inner]; n_obj >= 2 (n_obj == 1 returns the input, AEM:10-11). */
/* Alignment ("Pointer alignment" above): class 16: -; every other pointer class 4. */
int aoc_fg2bg_min(const float *dis, int n_obj, int n_ch, int64_t inner, int64_t dis_obj_stride,
                  float *out, int64_t out_obj_stride, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * k = 1 proxies / IA head: ATT:134-189 (calculate_attention_head[_for_eval]_p_m).
 *  Accumulates over n_frames maps  emb [n_frames, hw, C] (channel-last) with float label maps
 *  labels [n_frames, n_obj, hw] (the reference's one-hot [O,1,h,w] tensors; any float works), or
 *  [n_frames, hw, n_obj] when labels_pixel_major != 0 (the layout the matching functions take):
 *    pos[o] = sum_p emb[p] * label[o,p] / (sum_p label[o,p] + eps)
 *    neg[o] = (sum_p emb[p] - pos_sum[o]) / (sum_p (1 - label[o,p]) + eps)
 *  out_pos, out_neg [n_obj, C]; out_pos_sqnorm [n_obj] = |pos[o]|^2 (optional, may be NULL): the k = 1
 *  proxies go straight into aoc_proxy_corr_min's proxy table.
 */
size_t aoc_masked_mean_pool_workspace_bytes(int n_frames, int64_t hw, int n_obj, int C);
int aoc_masked_mean_pool(const float *emb, const float *labels, int n_frames, int64_t hw, int C,
                         int n_obj, int labels_pixel_major, float epsilon, float *out_pos, float *out_neg,
                         float *out_pos_sqnorm, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * FiLM gate: ATT:12-17 (IA_gate.forward) and CLB:81-84:
 *   gain[o,c] = 1 + tanh( sum_d head[o,d] * weight[c,d] + bias[c] );  y[o,c,:] = gain[o,c] * x[o,c,:]
 *  aoc_film_gain writes gain [n_obj, channels]; aoc_channel_scale streams x (in place allowed). */
int aoc_film_gain(const float *head, const float *weight, const float *bias, int n_obj,
                  int head_dim, int channels, float *gain, aoc_stream_t stream);
int aoc_channel_scale(const float *x, const float *gain, int64_t planes, int64_t hw, float *y,
                      aoc_stream_t stream);
/* Both steps in one launch (what IA_gate.forward does, ATT:12-17): x [n_obj, channels, hw]. */
int aoc_film_scale(const float *x, const float *head, const float *weight, const float *bias,
                   int n_obj, int head_dim, int channels, int64_t hw, float *y, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * conditioning_layer gate + pool: CL:23-43 (paper Eq. 7):
 *   s = phi(z) (1x1 conv C->1), t = k-th largest of s per sample (k = int(beta*H*W), exact radix
 *   select), mask = s > t (strict), gap[n,c] = mean over ALL HW of z[n,c,:] * mask.
 *  z [N, C, HW]; phi_w [C]; phi_b [1]; gap [N, C] out; scores [N, HW] / threshold [N] optional outs
 *  (may be NULL, then they live in the workspace).
 */
size_t aoc_cond_gate_pool_workspace_bytes(int N, int C, int64_t hw);
int aoc_cond_gate_pool(const float *z, int N, int C, int64_t hw, const float *phi_w,
                       const float *phi_b, int k_rank, float *gap, float *scores, float *threshold,
                       void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The same, also emitting plane_mean [N, C] = mean over HW of z[n,c,:] (CLB:68 avg_pool2d, the input of conditioning_block's inter-object
 * code) from the SAME pass that computes the scores: a conditioning block then reads its activation three times (scores + plane sums,
 * masked pooling, FiLM scale) instead of four.  plane_mean may be NULL. */
int aoc_cond_gate_pool_ex(const float *z, int N, int C, int64_t hw, const float *phi_w,
                          const float *phi_b, int k_rank, float *gap, float *plane_mean, float *scores,
                          float *threshold, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* Small dense layer used by the conditioning MLPs (CL:46, CLB:81): y[n,:] = x[n,:] W^T + b. */
int aoc_linear(const float *x, const float *weight, const float *bias, int N, int in_dim,
               int out_dim, float *y, aoc_stream_t stream);
/* out[p,:] = sum_o labels[p,o] * rows[o,:]: the per-pixel proxy map fed to local_matching_proxy
 * (aocnet.py:325).  labels [n, n_obj], rows [n_obj, C], out [n, C]. */
int aoc_label_mix(const float *labels, const float *rows, int64_t n, int n_obj, int C, float *out,
                  aoc_stream_t stream);
/* Global average pool of planes [planes, hw] -> [planes]  (CLB:68). */
int aoc_plane_mean(const float *x, int64_t planes, int64_t hw, float *out, aoc_stream_t stream);
/* out [n_obj, head_dim + channels] = head [n_obj, head_dim] extended with the inter-object code of the plane means [n_obj, channels]:
 * out[o, head_dim + c] = sum_o' px[o', c] - px[o, c]  (decoding_module.py:126-130, torch.cat([head, px.sum(0, keepdim=True) - px], 1)) */
int aoc_head_delta(const float *head, int head_dim, const float *plane_means, int n_obj, int channels, float *out, aoc_stream_t stream);

/* DynamicPreHead, decoding_module.py:228-240 (1x1 convolution n_in -> n_out, GroupNorm(n_groups), ReLU) applied to the
 * [n_obj, n_in, hw] proto-mask tensor, fused with the concatenation of aocnet.py:362: out [n_obj, C + n_out, hw] holds the
 * current-frame embedding emb_hwc [hw, C] (expanded over the objects, transposed to channel-first) in channels [0, C) and the
 * pre-head output in channels [C, C + n_out) -- the tensor CalibrationDecoding consumes.  emb_hwc may be NULL with C = 0.
 * weight [n_out, n_in], bias / gamma / beta [n_out]; GroupNorm statistics (biased variance) are reduced in a fixed order. */
size_t aoc_prehead_workspace_bytes(int n_obj, int n_out, int group_size, int64_t hw);
int aoc_prehead(const float *feat, int n_obj, int n_in, int64_t hw, const float *weight, const float *bias, int n_out,
                int n_groups, const float *gamma, const float *beta, float eps, const float *emb_hwc, int C, float *out,
                void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* conditioning_block codes in one launch, CLB:68-80: code[n] = [ W1 gap[n] + b1 | W2 (sum_m px[m] - px[n]) + b2 | W3 head[n] + b3 ]
 * with gap [N, C] (aoc_cond_gate_pool), px = plane means [N, C] (aoc_plane_mean), head [N, D]; W1, W2 [C, C], W3 [D, D] are
 * the mlp_layer weights of CL_1..CL_3 (row-major [out, in]); code [N, 2C + D] feeds aoc_film_scale. */
int aoc_cond_codes(const float *gap, const float *plane_means, const float *head, const float *w1, const float *b1,
                   const float *w2, const float *b2, const float *w3, const float *b3, int N, int C, int D,
                   float *code, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Decoder-side streams next to the FiLM gates.
 *
 * aoc_plane_reduce   out[plane] = sum over the plane of x (mode 0), x^2 (mode 1), |x| (mode 2)      (gct.py:19,27-30)
 * aoc_gct_gate       GCT gate of gct.py:17-36 from those sums [N, C]: l2 mode (l1_mode = 0, sums of squares) or l1 mode
 *                    (sums of x or |x|); gate [N, C] = 1 + tanh(embedding * norm + beta); y = x * gate is aoc_channel_scale
 * aoc_object_logit   IA_logit, decoding_module.py:151-160: out[n, p] = sum_c x[n, c, p] * weight[n * weight_stride + c] +
 *                    bias[n * bias_stride] (the per-object 1x1 grouped convolution with weights generated from the IA head;
 *                    weight / bias are usually views of one [N, C + 1] linear output: weight_stride = bias_stride = C + 1) */
int aoc_plane_reduce(const float *x, int64_t planes, int64_t hw, int mode, float *out, aoc_stream_t stream);
int aoc_gct_gate(const float *plane_sums, const float *alpha, const float *gamma, const float *beta, int N, int C,
                 float eps, int l1_mode, float *gate, aoc_stream_t stream);
int aoc_object_logit(const float *x, int N, int C, int64_t hw, const float *weight, int64_t weight_stride,
                     const float *bias, int64_t bias_stride, float *out, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The decoder's tail (csrc/decoder_tail.hip): the shortcut stage of decoder_final and the prediction head.  fp32, up to AOC_MAX_OBJECTS
 * objects (beyond: AOC_ERR_UNSUPPORTED); every argument is validated before the first launch (no device needed for a rejection).
 *
 * Bicubic resize = PyTorch's upsample_bicubic2d with align_corners=True (decoding_module.py:163): A = -0.75, four taps per axis at
 * floor(src) - 1 .. + 2 clamped to the map, src = o (in - 1) / (out - 1) (0 when out = 1).  The coordinate is split in integers
 * (tap index o (in - 1) div (out - 1), exact; fraction float(o (in - 1) mod (out - 1)) / float(out - 1), one rounding).
 *
 * Mean over the H x W map of the bicubic upsample of each coarse plane in [P, h, w], computed from the coarse plane alone
 * (decoding_module.py:163 + :172 for the upsampled channels): (1 / HW) sum_ij cy[i] cx[j] x[i, j], cy / cx = column sums of the two 1-D
 * interpolation matrices.  out [P]. */
int aoc_bicubic_plane_mean(const float *in, int64_t P, int h, int w, int H, int W, float *out, aoc_stream_t stream);
/* decoding_module.py:163 + :170 (+ the scaling of ATT:15-16) without the intermediate tensors: out [N, Ce + Cr, H, W] with
 *   out[n, c < Ce] = gain[n, c] * bicubic(x[n, c]),  out[n, Ce + c] = gain[n, Ce + c] * low[n, c];
 * x [N, Ce, h, w]; low [N, Cr, H, W] (NULL with Cr = 0: a plain plane resize); gain [N, Ce + Cr] or NULL (= 1). */
int aoc_bicubic_cat_scale(const float *x, const float *low, const float *gain, int N, int Ce, int Cr, int h, int w, int H, int W,
                          float *out, aoc_stream_t stream);
/* decoding_module.py:163 and :170-176 as one call without host synchronisation: plane means of the concatenation (the upsampled part from the
 * coarse map, the shortcut part low -- the branch after its ReLU, :168 -- through the plane-mean kernel), px1_delta appended to IA_head
 * [N, head_dim] (:173-176), IA10's gain (weight [Ce + Cr, head_dim + Ce + Cr], bias [Ce + Cr] or NULL; ATT:13-14) and the gated
 * concatenation out [N, Ce + Cr, H, W].  Optional outputs (NULL = not wanted): plane_means [N, Ce + Cr], gain [N, Ce + Cr]. */
size_t aoc_shortcut_stage_workspace_bytes(int N, int Ce, int Cr, int head_dim);
int aoc_shortcut_stage_enqueue(const float *x, const float *low, const float *IA_head, const float *weight, const float *bias, int N,
                               int Ce, int Cr, int head_dim, int h, int w, int H, int W, float *out, float *plane_means, float *gain,
                               void *workspace, size_t workspace_bytes, aoc_stream_t stream);
/* decoding_module.py:144-147 in one launch: IA_logit (:151-160) for the fg and bg heads and augment_background_logit (:213-225).
 * wb_fg, wb_bg: rows of [C weights | bias] per object, `stride` floats apart (the two IA_final outputs [N, C + 1]); x [N, C, hw] is read once.
 *   pred[n] = fg[n];  for N > 1: pred[0] += min over n >= 1 of bg[n]   (bg[0] is not computed; wb_bg may be NULL for N = 1)
 * pred [N, hw] is the reference's [1, N, h, w] (the permute of :224).  fg and bg are bit-equal to what the object-logit call gives. */
int aoc_logit_head(const float *x, const float *wb_fg, const float *wb_bg, int64_t stride, int N, int C, int64_t hw, float *pred,
                   aoc_stream_t stream);
/* augment_background_logit alone (decoding_module.py:213-225) for logits that already exist: fg, bg [N, hw] -> pred [N, hw] as above
 * (bg may be NULL for N = 1; pred may alias fg). */
int aoc_background_merge(const float *fg, const float *bg, int N, int64_t hw, float *pred, aoc_stream_t stream);

/* GroupNorm (+ residual) + ReLU of the decoder's Bottleneck (networks/layers/gct.py:69-90: bn1/bn2 followed by relu, bn3 followed by
 * `out += residual; relu`): y = [relu]( GroupNorm_groups(x) * gamma + beta [+ residual] ), x [N, C, hw], biased variance over each
 * group's channels x hw as torch.nn.GroupNorm.  Two streams over x (statistics, apply) and one write instead of the separate
 * normalisation / add / ReLU passes.  gamma, beta [C] or NULL; residual [N, C, hw] or NULL; y may alias x.
 * The workspace starts with the statistics, float [N * groups][2] = (mean, rstd) of each (sample, group), rounded to float once each:
 * aoc_groupnorm_relu_grad reads them from there (the training twin keeps the workspace instead of recomputing them). */
size_t aoc_groupnorm_relu_workspace_bytes(int N, int groups);
int aoc_groupnorm_relu(const float *x, int N, int C, int64_t hw, int groups, const float *gamma, const float *beta,
                       float eps, const float *residual, int relu, float *y, void *workspace,
                       size_t workspace_bytes, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The decoder's memory modulators, decoding_module.py:192-210 (Modulator_1 / Modulator_2): the concatenation with the memory fused into
 * gate 1, and gates 2 and 3 fused into the apply pass of the GroupNorm in front of them.  fp32.  The gain of both entry points is the
 * routine of aoc_film_scale (same summation order), so each returns exactly the bits of the composition it replaces.  Every argument is
 * validated before the first launch (no device needed for a rejection).
 *
 * torch.cat([x, mem], dim=1) (:193 / :203) + IA_gate (:194 / :204, ATT:12-17) in one launch; the concatenation is never written ungated:
 *   y[o, c < Cx] = g[o, c] * x[o, c],  y[o, Cx + c] = g[o, Cx + c] * mem[o, c],  g = 1 + tanh(head W^T + b) over the Cx + Cm channels.
 * x [n_obj, Cx, hw]; mem [n_obj, Cm, hw] (may alias x: the first frame of a sequence; NULL with Cm = 0, which is aoc_film_scale);
 * head [n_obj, head_dim]; weight [Cx + Cm, head_dim]; bias [Cx + Cm] or NULL; y [n_obj, Cx + Cm, hw].  Every source plane is read once and
 * y is written once, 16 bytes per lane whatever the 16-byte misalignments of the three base pointers are. */
int aoc_cat_film_scale(const float *x, const float *mem, const float *head, const float *weight, const float *bias, int n_obj,
                       int head_dim, int Cx, int Cm, int64_t hw, float *y, aoc_stream_t stream);
/* aoc_groupnorm_relu followed by IA_gate (gct.py:84-90 + decoding_module.py:196,198 / :206,208) with the gate folded into the apply pass:
 *   y = g[n, c] * [relu]( GroupNorm_groups(x) * gamma + beta [+ residual] ),  g = 1 + tanh(head W^T + b);
 * head [N, head_dim]; weight [C, head_dim]; gate_bias [C] or NULL; everything else, the statistics pass and the workspace
 * (aoc_groupnorm_relu_workspace_bytes) as aoc_groupnorm_relu.  y may alias x. */
int aoc_groupnorm_relu_scale(const float *x, int N, int C, int64_t hw, int groups, const float *gamma, const float *beta,
                             float eps, const float *residual, int relu, const float *head, const float *weight,
                             const float *gate_bias, int head_dim, float *y, void *workspace, size_t workspace_bytes,
                             aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ASPP, networks/layers/aspp.py:7-70 (the module CalibrationDecoding runs between IA9 and Modulator_1, decoding_module.py:53, :131): what is
 * not a convolution.  fp32.  Every argument is validated before the first launch (no device needed for a rejection).  Pointer lists are HOST
 * arrays of at most 8 device pointers; they are copied into the kernel's arguments, so the array may be freed when the call returns.
 *
 * One pass over x [planes, hw]: sum[p] = sum of x, sumsq[p] = sum of x^2, mean[p] = sum[p] / (float)hw.  Replaces the four
 * x.pow(2).sum((2, 3)) of aspp.py:19 (via gct.py:19: aspp1..4.GCT read the same x) and the AdaptiveAvgPool2d of aspp.py:46.  Any of the three
 * outputs may be NULL, not all of them.  Fixed summation order, no atomics: the same bits on every run (the order follows the 16-byte
 * alignment of x's planes, so "the same" includes the base pointer modulo 16). */
int aoc_plane_sum_sumsq(const float *x, int64_t planes, int64_t hw, float *sum, float *sumsq, float *mean, aoc_stream_t stream);
/* aoc_gct_gate for n_sets parameter sets over one plane_sums [N, C] in one launch (the gates of aspp1..4.GCT, aspp.py:19 via gct.py:17-34):
 * alpha, gamma, beta [n_sets, C]; gate [n_sets, N, C]; set k carries exactly the bits of aoc_gct_gate with row k of the parameters. */
int aoc_gct_gate_multi(const float *plane_sums, const float *alpha, const float *gamma, const float *beta, int n_sets, int N, int C,
                       float eps, int l1_mode, float *gate, aoc_stream_t stream);
/* y_k[p, :] = gains[k, p] * x[p, :] for k < n_out <= 8 with x [planes, hw] read once (the x * gate of gct.py:36 for aspp1..4.GCT, aspp.py:19):
 * gains [n_out, planes]; y_ptrs: n_out pointers to [planes, hw].  Each y_k carries the bits of aoc_channel_scale.  16 bytes per lane whatever
 * the 16-byte misalignments of x and of the y_k are.  y_0 may be x itself when n_out == 1; every other overlap is rejected. */
int aoc_channel_scale_multi(const float *x, const float *gains, int n_out, int64_t planes, int64_t hw, float *const *y_ptrs,
                            aoc_stream_t stream);
/* aspp.py:21-23 for the four branches and the concatenation of :62-63 as a statistics launch and an apply launch:
 *   y[n, k C_src + c]     = [relu]( GroupNorm_groups(x_k)[n, c] * gamma[k, c] + beta[k, c] )     k < n_src <= 8
 *   y[n, n_src C_src + c] = [relu]( tail[n, c] )  over the whole plane                            c < C_tail
 * x_ptrs: n_src pointers to [N, C_src, hw]; gamma, beta [n_src, C_src] or NULL; tail [N, C_tail] (NULL with C_tail = 0) is the pooled branch of
 * :61 -- F.interpolate(..., align_corners=True) from a 1 x 1 map (:62) is a broadcast, the expanded tensor is never materialised;
 * y [N, n_src C_src + C_tail, hw] overlaps no input (x_k, tail, gamma, beta), nor plane_sumsq or the workspace, which overlap nothing either
 * (all checked: AOC_ERR_INVALID_ARG).  The statistics are those of aoc_groupnorm_relu (same routine, every source in one
 * launch), so y carries the bits of torch.cat([aoc_groupnorm_relu(x_k) ..., tail expanded], 1).  plane_sumsq [N, n_src C_src + C_tail] (may be
 * NULL) = sum over each plane of y^2, accumulated from the values being stored in a fixed order: the plane sums GCT(640) needs (:65 via
 * gct.py:19) without another read of y; deterministic (for one alignment of y modulo 16), not the bits of aoc_plane_reduce. */
size_t aoc_groupnorm_cat_relu_workspace_bytes(int n_src, int N, int groups);
int aoc_groupnorm_cat_relu(const float *const *x_ptrs, int n_src, int N, int C_src, int64_t hw, int groups, const float *gamma,
                           const float *beta, float eps, const float *tail, int C_tail, int relu, float *y, float *plane_sumsq,
                           void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Eval-loop memory policy (the caller of the matching path).
 *
 * aoc_confident_labels: the per-pixel decision of one frame, eval_manager_mm.py:253-265,300-326,339-346,357-361 with
 *   shannon_entropy.py:10-13.   probs [n_ch, n] = the (augmentation-averaged) class probabilities;
 *   exist_bits: bit c = label c has appeared in a ground-truth map so far (other channels are zeroed);
 *   join_label [n] or NULL: ground truth that introduces new objects (0 = keep the prediction, < 0 = unsure);
 *   labels_out [n] = argmax (first maximum) with the join override; confident_out [n] (may be NULL) = the same label or
 *   125 where the entropy -sum p log(p + 1e-6) over the seen channels exceeds unc_ratio; entropy_out [n] (may be NULL).
 * aoc_label_onehot_nearest: aocnet.py:128-133,151: nearest-neighbour resize of an int label map [H, W] to [h, w] and
 *   one-hot over n_obj ids -> float [h, w, n_obj] (label 125 or any id >= n_obj matches nothing: an all-zero row). */
int aoc_confident_labels(const float *probs, int n_ch, int64_t n, uint32_t exist_bits, const int32_t *join_label,
                         float unc_ratio, int32_t *labels_out, int32_t *confident_out, float *entropy_out,
                         aoc_stream_t stream);
int aoc_label_onehot_nearest(const int32_t *label, int H, int W, int h, int w, int n_obj, float *onehot_hwc,
                             aoc_stream_t stream);

/* Test-time augmentation (--flip / --ms of tools/eval_net_mm_rpa.py:21-23 -> cfg.TEST_FLIP, cfg.TEST_MULTISCALE): the tail of one frame of
 * eval_manager_mm.py:196-361 for a LIST of augmented samples as ONE launch.  Per output pixel (y, x), in the reference's order:
 *   1. for each augmentation a, in order: p_a[c] = softmax_c(bilinear_{align_corners=True}(logits_a)[c]) (aocnet.py:103-106) taken at (y, x), or at
 *      (y, W - 1 - x) when flip[a] (the planes are those of the horizontally mirrored image, :285-286); channels whose bit of exist_bits[a] is
 *      clear become 0 AFTER the soft-max, without renormalisation (:253-265);
 *   2. s[c] = sum_a p_a[c] in fp32, in augmentation order; label = first maximum of s (torch.argmax of the mean, :318-320), then the join_label
 *      override of aoc_confident_labels (:321-326);
 *   3. entropy -sum_{c seen} p log(p + 1e-6) (shannon_entropy.py:10-13), "seen" = exist_bits of the last augmentation:
 *      mode 0 (reference): p = the LAST augmentation's probabilities at (y, x) in ITS OWN orientation, not flipped back -- all_pred_exist is built
 *      before the flip of :286, and :306 / :339 read what the last loop iteration left;   mode 1 (consistent): p = s / n_aug.
 *      Then the join_label terms and > unc_ratio -> 125 as in aoc_confident_labels (:339-346, :357-361);
 *   4. outputs, each optional (NULL = not written; at least one): label, confident, label_flipped[y, x] = label[y, W - 1 - x] (:327-329),
 *      confident_flipped (mode 1 only), entropy, mean_probs [n_ch, H, W] = s / n_aug.
 * exist_bits is per augmentation because the reference updates label_all_list INSIDE its augmentation loop (:268-272): on a frame whose ground
 * truth introduces an object, augmentation 0 still zeroes that channel and the later ones do not.  Every other caller passes n_aug equal values.
 * With n_aug = 1 and no flip the call is interpolate -> softmax -> aoc_confident_labels in one launch.  n_aug <= AOC_MAX_TTA_AUGS (eight scales
 * with their flipped twins), n_ch <= 32 (beyond: AOC_ERR_UNSUPPORTED); everything is validated before the launch. */
#define AOC_MAX_TTA_AUGS 16
typedef struct aoc_tta_desc {
    int32_t n_aug, n_ch;             /* augmentations, channels (objects incl. background) */
    int32_t H, W;                    /* output (image) size */
    int32_t mode;                    /* 0 = reference, 1 = consistent (see 3.) */
    float unc_ratio;
    int32_t h[AOC_MAX_TTA_AUGS], w[AOC_MAX_TTA_AUGS];    /* size of augmentation a's logit planes */
    int32_t flip[AOC_MAX_TTA_AUGS];                      /* 0 / 1 */
    uint32_t exist_bits[AOC_MAX_TTA_AUGS];               /* bit c = label c has appeared in a ground-truth map (aoc_confident_labels) */
    float scale_h[AOC_MAX_TTA_AUGS], scale_w[AOC_MAX_TTA_AUGS];   /* set by the call ((h - 1) / (H - 1), ...): the caller's values are ignored */
    int64_t plane_stride[AOC_MAX_TTA_AUGS];              /* floats between two channels' planes, >= h * w */
    const float *logits[AOC_MAX_TTA_AUGS];               /* [n_ch] planes of [h, w] float32, row-major */
    const int32_t *join_label;       /* [H, W] or NULL (aoc_confident_labels) */
    int32_t *label, *confident, *label_flipped, *confident_flipped;   /* [H, W] each, or NULL */
    float *entropy;                  /* [H, W] or NULL */
    float *mean_probs;               /* [n_ch, H, W] or NULL */
} aoc_tta_desc;
int aoc_tta_merge(const aoc_tta_desc *desc, aoc_stream_t stream);

/* J (region similarity) and F (boundary measure) of a predicted label map against the ground truth, summed over the foreground
 * objects 1 .. n_obj-1 and ACCUMULATED on the device: accum[0] += sum_o J_o, accum[1] += sum_o F_o,
 * accum[2] += n_obj - 1, accum[3] += 1.  The reference scores saved PNGs with the external DAVIS toolkit (README.md:110; its only
 * in-repo IoU is utils/metric.py:3-34): the definitions here are DAVIS-2017's db_eval_iou and db_eval_boundary (seg2bmap boundaries,
 * dilation by skimage's disk(bound_pix), bound_pix = ceil(0.008 * hypot(H, W)) chosen by the caller).  pred, gt [H, W] int32 labels;
 * workspace_is_clean != 0 skips the zeroing of the counters (the call leaves them zeroed).  n_obj <= 16. */
size_t aoc_mask_jf_workspace_bytes(int H, int W);
int aoc_mask_jf_accumulate(const int32_t *pred, const int32_t *gt, int H, int W, int n_obj, int bound_pix,
                           void *workspace, size_t workspace_bytes, int workspace_is_clean, double *accum,
                           aoc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One frame as ONE call: the counterpart of AOCNet.before_seghead_process (networks/aoc/aocnet.py:114-372, eval branch, batch 1) up to the
 * tensor handed to DynamicPreHead (aocnet.py:355-358) and the attention head (aocnet.py:297), enqueued on `stream` without any host
 * synchronisation.  It issues the kernels of the individual entry points above (results bit-identical to calling them one by one, which
 * is what hotpath.proto_mask_features does) out of ONE caller-owned device workspace per sequence, and keeps across the frames of a sequence
 * what only depends on the reference pool: its fp16 split records (append-only pool: only new frames are converted), the pooled reference
 * heads (ATT:155-170) and the dense kernel's plan -- keyed by pool_key.
 *
 * Covered configuration: C = 100, <= 30 objects (AOC_MAX_OBJECTS; beyond 16 the dense matching takes the exact-fp32 kernel in slices of 16 and
 * the correlation the non-record entry point, as hotpath.proto_mask_features does), and every switch the reference's evaluation CLI / config
 * exposes: MODEL_FLOAT16_MATCHING, MODEL_LOCAL_DOWNSAMPLE on / off, TEST_LOCAL_ATROUS_RATE, TEST_GLOBAL_ATROUS_RATE (round 5; the default
 * configuration -- fp32, down-sampled local matching, atrous rates 1, <= 16 objects -- keeps the fused launches of round 4, the others go
 * through the individual entry points the drop-in mirrors use, in the same order: results equal theirs).  Other widths return AOC_ERR_UNSUPPORTED.
 *
 * The adaptive proxies (k-means chain, AEM:252-286: aoc_label_prep, aoc_kmeans_replicate_levels, aoc_kmeans_segmented_rep,
 * aoc_build_proxies) only depend on the pool and are produced by the caller on ANOTHER stream, ahead of the frame; this call gets the label
 * prep arrays, the proxy table they are written to, and two hipEvent_t: it waits for prep_ready before reading the label prep and for
 * proxies_ready in front of the correlation launch (NULL = already ordered on `stream`).
 *
 * Output channels of feat [n_obj, n_ch, h, w], n_ch = aoc_frame_channels(): global(1) | cluster (centroid, centroid_avg) per level |
 * proxy(1) | local(n_radii) | local_proxy(n_radii) | prev_mask(1) [| local_bg(n_radii) | global_bg(1)]. */
/* Alignment ("Pointer alignment" above): class 16: ref_emb, match_emb, prev_emb, cur_emb, proxy_table; every other pointer class 4. */
typedef struct aoc_frame_desc {
    int32_t h, w, C, n_obj;          /* map size, embedding width, objects incl. background */
    int32_t R, R_capacity;           /* pool frames this frame sees / the workspace was sized for */
    int32_t n_radii, radii[8];       /* MODEL_MULTI_LOCAL_DISTANCE */
    int32_t n_levels, levels[8];     /* cluster_num per level (AEM:232; one level: {16}) */
    int32_t kmax;                    /* max(levels): proxy slots per (level, object, set) in the table */
    int32_t matching_background;     /* MODEL_MATCHING_BACKGROUND */
    int32_t n_adaptive;              /* = n_levels * n_obj * 2 * kmax rows of the proxy table in front of the n_obj k = 1 rows */
    float epsilon;                   /* MODEL_EPSILON */
    int32_t pool_prefix_frames;      /* how many leading pool frames are UNCHANGED since the previous call on this state: their split records are
                                        kept, the frames behind them are converted again.  Append-only pool: R (or anything >= the previous R);
                                        a pool whose frames were replaced: the first replaced frame's index; 0 converts everything */
    int32_t stream_cus;              /* CUs `stream` may use when the caller created it with a HIP CU mask: the matrix kernels of THIS call size their
                                        grids in whole rounds of that many CUs; 0 = the process-wide aoc_set_stream_cus value */
    /* the switches the reference's evaluation CLI / config exposes (tools/eval_net_mm_rpa.py:9-35, configs/resnet101_aocnet.py:71,78,125,126) */
    int32_t float16_matching;        /* MODEL_FLOAT16_MATCHING (--float16): the reference's `.half()` arithmetic for the dense, k = 1 proxy and local
                                        matchings; the cluster channels are the constant 1 the reference degrades to */
    int32_t local_downsample;        /* MODEL_LOCAL_DOWNSAMPLE: local matching at (h / 2 + 1, w / 2 + 1) (1) or at full resolution (0) */
    int32_t local_atrous_rate;       /* TEST_LOCAL_ATROUS_RATE (>= 1) */
    int32_t match_hw;                /* TEST_GLOBAL_ATROUS_RATE > 1 (--global_atrous_rate): rows per pool frame of match_emb (the pool sub-sampled on the
                                        atrous grid, AEM:533-579: every rate-th row and column); 0 = the matching pool is ref_emb itself */
    int64_t pool_key;                /* != 0; changes whenever the pool's content changes (append-only pool: R).  Keys the pooled reference
                                        heads and the dense kernel's plan */
    const float *ref_emb;            /* [R * h * w, C]   reference pool, resident, append-only */
    const float *ref_labels;         /* [R * h * w, n_obj] float 0 / 1 */
    const float *match_emb;          /* [R * match_hw, C] the pool the dense and cluster matchings see when match_hw > 0 (aoc_atrous_subsample of every
                                        pool frame; the label-prep arrays below then index ITS rows); NULL with match_hw = 0.  The pooled heads
                                        (attention head, k = 1 proxies) always come from ref_emb / ref_labels (aocnet.py:297) */
    const float *prev_emb, *prev_labels, *cur_emb;     /* [h * w, C], [h * w, n_obj], [h * w, C] */
    const float *dis_bias;           /* [n_obj] */
    const uint32_t *right_bits, *wrong_bits;           /* aoc_label_prep(ref_labels) */
    const int32_t *fg_rows, *obj_rows, *counts, *obj_offsets;
    float *proxy_table;              /* [n_adaptive + n_obj, C]: adaptive rows by the k-means chain, k = 1 rows by this call */
    float *proxy_sqnorm;             /* [n_adaptive + n_obj] */
    void *prep_ready, *proxies_ready;                  /* hipEvent_t or NULL */
    float *feat;                     /* [n_obj, n_ch, h, w] */
    float *head;                     /* [n_obj, 4 C] */
    void *probe[6];                  /* measurement only, hipEvent_t or NULL: recorded on `stream` immediately before / after the dense matching
                                        op [0][1], the correlation launch [2][3], the local-matching launch [4][5] */
} aoc_frame_desc;
/* Host-side record of what the workspace holds; caller-owned, zero-initialised when a sequence starts (the library keeps no state). */
typedef struct aoc_seq_state {
    int64_t initialised, records_frames, ref_pool_key, plan_key, plan_rows;
    int64_t corr_tables_key;         /* the correlation passes' tile tables the workspace holds (aoc_proxy_corr_min_records_cached) */
} aoc_seq_state;
int aoc_frame_channels(int n_radii, int n_levels, int matching_background);
size_t aoc_frame_workspace_bytes(int h, int w, int C, int n_obj, int R_capacity, int n_radii, int n_levels);
/* Alignment ("Pointer alignment" above): class 16: workspace; every other pointer class 4. */
int aoc_frame_enqueue(const aoc_frame_desc *desc, aoc_seq_state *state, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The adaptive proxies of the frames that see ONE pool state as ONE call (round 5): what hotpath.launch_cluster_proxies_batch issued as
 * three C calls plus a dozen tensor allocations and 2 F table copies -- aoc_kmeans_replicate_levels, aoc_kmeans_segmented_rep (20 Lloyd
 * iterations, AEM:252-279), aoc_build_proxies (AEM:280-282) and the scatter of every frame's proxies into ITS proxy table -- out of one
 * caller-owned workspace, enqueued on `stream` (the caller's side stream) without host synchronisation.  Bit-identical to the three calls.
 * With aoc_frame_enqueue and aoc_gates_enqueue a frame of the orchestrated path is three C calls (one per stream it touches). */
/* Alignment ("Pointer alignment" above): class 16: pool, tables; every other pointer class 4. */
typedef struct aoc_chain_desc {
    int32_t C, n_obj, n_frames;      /* embedding width, objects incl. background, frames F that see this pool state (<= 8) */
    int32_t n_levels, levels[8];     /* cluster_num per level (AEM:232) */
    int32_t kmax, iters;             /* max(levels); Lloyd iterations (20: scipy's kmeans2 default the reference uses) */
    int32_t reserved0;
    int64_t pool_rows;               /* rows of the pool the matchings see (R * h * w, or R * match_hw on the atrous grid) */
    int64_t rows_capacity;           /* entries of obj_rows (aoc_label_prep: pool_rows * n_obj) */
    const float *pool;               /* [pool_rows, C] */
    const int32_t *fg_rows, *obj_rows, *obj_offsets;    /* aoc_label_prep of that pool's labels */
    const int32_t *init_rows;        /* [n_frames * n_levels * n_obj, kmax] segment-local initial rows, (frame, level, object)-major */
    float *tables[8];                /* per frame: its proxy table [n_levels * n_obj * 2 * kmax + n_obj, C]; the adaptive rows are written */
    float *sqnorms[8];               /* per frame: [n_levels * n_obj * 2 * kmax + n_obj] */
} aoc_chain_desc;
size_t aoc_cluster_chain_workspace_bytes(const aoc_chain_desc *desc);
/* byte offsets (into the workspace) of what the chain leaves there, for callers that want to look at it: [0] centroids [S, kmax, C] float,
 * [1] labels [n_frames * n_levels * rows_capacity] int32, [2] cluster counts [S, kmax] int32, [3] proxies [S, 2, kmax, C] float,
 * [4] proxy squared norms [S, 2, kmax] float, [5] seg_k [S] int32, [6] seg_offsets [S + 1] int32;  S = n_frames * n_levels * n_obj */
int aoc_cluster_chain_layout(const aoc_chain_desc *desc, int64_t *offsets7);
/* Alignment ("Pointer alignment" above): class 16: workspace; every other pointer class 4. */
int aoc_cluster_chain_enqueue(const aoc_chain_desc *desc, void *workspace, size_t workspace_bytes, aoc_stream_t stream);

/* The modulation gates of CalibrationDecoding.forward (decoding_module.py:96-149, 162-210) as ONE call: a list of gate descriptors, every
 * gate issuing exactly the launches of its module mirror (outputs bit-identical to attention.IA_gate / conditioning_layer.conditioning_block).
 *   kind 0  IA_gate (ATT:7-17):                       y = x * (1 + tanh(head W^T + b)),                     W [channels, head_dim]
 *   kind 1  IA gate with the extended head (decoding_module.py:126-130): head' = (head | sum_o GAP(x) - GAP(x)), W [channels, head_dim + channels]
 *   kind 2  conditioning_block (CLB:50-86):  W = mlp_layer.weight [channels, 2 channels + head_dim]; phi = CL_1.phi_layer; w1..b3 = the
 *           mlp_layer of CL_1 / CL_2 / CL_3; k_rank = int(beta * H * W) (CL:32)
 * x, y [n_obj, channels, hw]; head [n_obj, head_dim]; the scratch of all gates comes out of one workspace (stream-ordered reuse). */
typedef struct aoc_gate_desc {
    int32_t kind, channels, k_rank, reserved;
    int64_t hw;
    const float *x;
    float *y;
    const float *w, *b;
    const float *phi_w, *phi_b, *w1, *b1, *w2, *b2, *w3, *b3;
    void *probe[4];                  /* measurement only, hipEvent_t or NULL: recorded immediately before / after the gate's aoc_film_scale [0][1]
                                        and its aoc_cond_gate_pool_ex [2][3] */
} aoc_gate_desc;
size_t aoc_gates_workspace_bytes(const aoc_gate_desc *gates, int n_gates, int n_obj, int head_dim);
int aoc_gates_enqueue(const aoc_gate_desc *gates, int n_gates, const float *head, int n_obj, int head_dim, void *workspace, size_t workspace_bytes,
                      aoc_stream_t stream);

/*
 * Training criterion (csrc/loss_grad.hip; aoc_amd.loss_train): aocnet.py:71-82 and Concat_CrossEntropyLoss (networks/layers/loss.py:52-97) for
 * ONE sample, without the upsampled logits: bilinear upsample (align_corners=True) + per-pixel cross-entropy + argmax, the mean of the k
 * hardest pixels, the mask of those pixels, and the gradient with respect to the coarse logits.  pred [C, h, w] float32, C = 1 .. 31 (other
 * values: AOC_ERR_UNSUPPORTED); labels [H * W] int32; H * W and C * h * w below 2^31.  fp32, no float atomics, every float sum in an order
 * fixed by the shapes (the same buffers give the same bits); every argument is validated before the first launch and a rejected call
 * writes nothing; every pointer marked optional may be NULL, and each optional output has the same bits alone as with the others.
 *
 * The tap of fine index o on an axis of `in` coarse and `out` fine points (torch's upsample_bilinear2d, align_corners=True, in float):
 *   scale = (float)(in - 1) / (float)(out - 1)  (0.0f when out == 1);  src = (float)o * scale;  i0 = min((int)src, in - 1);
 *   i1 = min(i0 + 1, in - 1);  w1 = min(max(src - (float)i0, 0), 1);  w0 = 1.0f - w1
 * and the logit x_c = w0y * (w0x * a + w1x * b) + w1y * (w0x * c + w1x * d), a, b the taps of row i0y and c, d of row i1y; a tap whose
 * weight is exactly 0 is not multiplied in, so h == H and w == W hands the logits through bit for bit.
 *
 * aoc_upsample_ce_forward: m = max_c x_c (the lowest channel of a tie is argmax), lse = m + logf(sum_c expf(x_c - m)) with the channels in
 * ascending order, loss = lse - x[label] (never negative).  A pixel whose label is ignore_index, or lies outside [0, C), gets loss +0.0f;
 * the second kind is counted in bad[0] (an integer atomic into a word the call zeroes first).  valid_partial[b] = the pixels of
 * [256 b, 256 b + 256) with a label in [0, C) other than ignore_index; aoc_upsample_ce_partials(H * W) entries.  loss, lse [H * W] float,
 * argmax [H * W] int32, valid_partial, bad: all optional. */
int64_t aoc_upsample_ce_partials(int64_t n);
int aoc_upsample_ce_forward(const float *pred, const int32_t *labels, int C, int h, int w, int H, int W, int ignore_index, float *loss, float *lse,
                            int32_t *argmax, int32_t *valid_partial, int32_t *bad, aoc_stream_t stream);
/* aoc_topk_mean: loss [n] (n < 2^31), 1 <= k <= n (else AOC_ERR_INVALID_ARG) -> thr = the k-th largest value (a radix select over the
 * monotone integer image of the floats: four passes of eight bits, many workgroups, integer histograms), n_gt = the number of values
 * strictly above thr, mean = (S + (float)(k - n_gt) * thr) / (float)k with S the sum of the values above thr: contiguous chunks of
 * max(4096, ceil(n / 1024) rounded up to 256) values; in a chunk thread t of 256 adds elements t, t + 256, ... in ascending order, the xor
 * butterfly over a wave, the four wave sums in ascending order; then the chunks in ascending order from 0.0f.  A NaN is always added, so it
 * makes mean NaN (nothing else is promised then).  mean, thr, n_gt are single device words, each optional.
 * aoc_valid_mean (the reduction='mean' branch): mean = S / (float)n_valid, S over every value in the same order, n_valid = the sum of
 * aoc_upsample_ce_forward's n_partial counts; 0 valid pixels give 0 / 0 = NaN, as torch does.  Workspace: aoc_topk_mean_workspace_bytes(n). */
size_t aoc_topk_mean_workspace_bytes(int64_t n);
int aoc_topk_mean(const float *loss, int64_t n, int64_t k, float *mean, float *thr, int32_t *n_gt, void *workspace, size_t workspace_bytes,
                  aoc_stream_t stream);
int aoc_valid_mean(const float *loss, int64_t n, const int32_t *valid_partial, int64_t n_partial, float *mean, int32_t *n_valid, void *workspace,
                   size_t workspace_bytes, aoc_stream_t stream);
/* aoc_topk_select_mask: mask[p] (one byte, 0 / 1) = loss[p] > thr, or loss[p] == thr and fewer than k - n_gt pixels of that value stand at
 * lower indices: the lowest index wins a tie, and exactly k bytes are set.  thr, n_gt: the device words aoc_topk_mean wrote.
 * aoc_valid_mask (the reduction='mean' branch): mask[p] = labels[p] != ignore_index and lies in [0, C). */
size_t aoc_topk_select_mask_workspace_bytes(int64_t n);
int aoc_topk_select_mask(const float *loss, int64_t n, int64_t k, const float *thr, const int32_t *n_gt, uint8_t *mask, void *workspace,
                         size_t workspace_bytes, aoc_stream_t stream);
int aoc_valid_mask(const int32_t *labels, int64_t n, int C, int ignore_index, uint8_t *mask, aoc_stream_t stream);
/* aoc_criterion_forward: the forward of one sample as ONE call: aoc_upsample_ce_forward, then aoc_topk_mean and aoc_topk_select_mask (k >= 1) or
 * aoc_valid_mean and aoc_valid_mask (k == 0), exactly those launches with thr, n_gt and the valid counts kept in the workspace, so every output
 * has the bits of the separate calls.  loss [H * W] and mean are required; lse, argmax, mask [H * W] bytes, n_valid (written when k == 0) and bad
 * are optional.  Every argument is validated before the first launch. */
size_t aoc_criterion_forward_workspace_bytes(int64_t n);
int aoc_criterion_forward(const float *pred, const int32_t *labels, int C, int h, int w, int H, int W, int ignore_index, int64_t k, float *loss, float *lse,
                          int32_t *argmax, uint8_t *mask, float *mean, int32_t *n_valid, int32_t *bad, void *workspace, size_t workspace_bytes,
                          aoc_stream_t stream);
/* aoc_upsample_ce_grad: grad_pred [C, h, w] = U^T[ mask * scale * (softmax - onehot) ], scale = grad_out[0] / (float)k (k >= 1) or
 * grad_out[0] / (float)n_valid[0] (k == 0); grad_out, n_valid are device words, so nothing synchronises.  softmax_c = expf(x_c - lse) with
 * x_c by the forward's own expression, g = scale * (softmax_c - 1.0f) at the label's channel and scale * softmax_c elsewhere; pixels whose
 * label is ignore_index or out of range contribute nothing even when the mask selects them.  The adjoint is in gather form: a workgroup
 * owns a band of coarse rows of one channel (the channels are independent once lse is known); u[I, j] adds the fine columns J in ascending
 * order, tap 0 then tap 1 of each, grad[i, j] the fine rows I in ascending order likewise, each product rounded and then added from 0.0f; a
 * tap of weight 0 is skipped as in the forward.  A coarse pixel no fine pixel reaches is written as 0.  Nothing of size C * H * W is
 * written and no workspace is needed. */
int aoc_upsample_ce_grad(const float *pred, const int32_t *labels, const float *lse, const uint8_t *mask, const float *grad_out, int64_t k,
                         const int32_t *n_valid, int C, int h, int w, int H, int W, int ignore_index, float *grad_pred, aoc_stream_t stream);

/*
 * Training-time DynamicPreHead (csrc/prehead_grad.hip; aoc_amd.prehead_train): the backward of aoc_prehead, i.e. of decoding_module.py:228-240
 * (`x = self.conv(x); x = self.bn(x); x = self.relu(x)`) with the concatenation of aocnet.py:360-362 (`pre_to_cat = self.dynamic_prehead(
 * pre_to_cat)`, `torch.cat((to_cat_current_frame_embedding, pre_to_cat), 1)`, the embedding expanded over the objects at aocnet.py:188).
 * fp32, no float atomics, every sum in an order fixed by the shapes alone (no pointer alignment enters); two runs on the same buffers give the
 * same bits.  The limits and their status codes are aoc_prehead's: n_in <= 32, n_out <= 128, n_out % n_groups == 0, n_obj <= 65535, and an
 * embedding pointer that contradicts C (here: grad_emb_hwc != NULL with C == 0) -> AOC_ERR_UNSUPPORTED; a NULL required pointer or a
 * non-positive size -> AOC_ERR_INVALID_ARG; a short workspace -> AOC_ERR_WORKSPACE.  The grids add hw <= 2^37 and C <= 65535 * 32 (beyond:
 * AOC_ERR_UNSUPPORTED).  A rejected call enqueues nothing.
 *
 * grad_out [n_obj, C + n_out, hw] is the cotangent of aoc_prehead's out; feat [n_obj, n_in, hw] its input; stats [n_obj * n_groups][2] the
 * float32 (mean, rstd) aoc_prehead left in its workspace (behind n_obj * n_groups * n_chunks * 16 bytes rounded up to a multiple of 256,
 * n_chunks = ceil(hw / 256)); weight [n_out, n_in], bias, gamma, beta [n_out].  For object o, channel c of group g, pixel p, M = (n_out / n_groups) * hw:
 *   y    = fmaf(w[c,n_in-1], x[n_in-1], ... fmaf(w[c,0], x[0], bias[c]))           aoc_prehead's chain: bias first, k ascending
 *   xhat = (y - mean) * rstd          v = xhat * gamma[c] + beta[c]                aoc_prehead's own expression, one rounding per operation
 *   dz   = grad_out[o, C + c, p] where v > 0, else 0.0f                            (a select: the forward output's own `> 0`, bit for bit)
 *   SA[o,c] = sum_p dz                SB[o,c] = sum_p fl(dz * xhat)                in double: per chunk of 256 pixels eight runs (run j: the pixels
 *                                                                                  4 (j + 8 m) .. + 3, m = 0 .. 7, ascending), the eight by xor butterfly
 *                                                                                  (4, 2, 1); then the chunks, dealt to 64 sums (sum l: the chunks l,
 *                                                                                  l + 64, ... ascending), the 64 by xor butterfly (32 .. 1)
 *   grad_beta[c]  = (float) sum_o SA[o,c]       grad_gamma[c] = (float) sum_o SB[o,c]             double, the (object, chunk) pairs dealt to 64 sums likewise
 *   c1[o,g] = (float)(sum_{c in g} (double)gamma[c] * SA[o,c] / M)      c2[o,g] likewise from SB  double, c ascending from 0.0; M as a double
 *   dy   = rstd * ((gamma[c] * dz - c1) - xhat * c2)                               float32, one rounding per operation
 *   grad_feat[o,k,p] = fmaf(w[n_out-1,k], dy_{n_out-1}, ... fmaf(w[0,k], dy_0, 0.0f))             c ascending
 *   P[o,chunk,c,k]   = fmaf(dy_p, x_k[p], ...) over the chunk's 256 pixels, p ascending from 0.0f; P[o,chunk,c,n_in] the same with x = 1.0f
 *   grad_weight[c,k] = (float) sum_{o,chunk} (double)P[o,chunk,c,k]     grad_bias[c] = (float) sum_{o,chunk} (double)P[o,chunk,c,n_in]
 *                      double; the (object, chunk) pairs i = 0, 1, ... dealt to four sums s = i mod 4, each ascending, then ((s0 + s1) + s2) + s3
 *   grad_emb_hwc[p,k] = sum_o grad_out[o,k,p]                                      float32, o ascending from 0.0f
 * Every output is optional (NULL: its work is skipped) and has the same bits alone as with the others: the plane pass and the traversal do
 * not depend on what is asked for.  grad_emb_hwc [hw, C] is channel-last like emb_hwc and must be NULL when C == 0.  No mask, y, xhat or dy
 * tensor is stored: five launches (plane pass, the small sums, apply pass, the reduction of P, the embedding's transposing sum) read the
 * n_out channels of grad_out and feat twice and the embedding's channels once.  The workspace holds SA / SB per chunk, (c1, c2) and P
 * (n_obj * n_chunks * n_out * (n_in + 1) floats); it is needed unless grad_emb_hwc is the only output. */
size_t aoc_prehead_grad_workspace_bytes(int n_obj, int n_in, int n_out, int n_groups, int64_t hw);
int aoc_prehead_grad(const float *grad_out, const float *feat, const float *stats, const float *weight, const float *bias, const float *gamma,
                     const float *beta, int n_obj, int n_in, int n_out, int n_groups, int64_t hw, int C, float *grad_feat, float *grad_weight,
                     float *grad_bias, float *grad_gamma, float *grad_beta, float *grad_emb_hwc, void *workspace, size_t workspace_bytes,
                     aoc_stream_t stream);

/*
 * The training update (csrc/optim.hip; aoc_amd.optim_train): the lines of the reference trainer between loss.backward() and the next forward,
 *   train_manager_mm.py:283       torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.TRAIN_CLIP_GRAD_NORM)
 *   train_manager_mm.py:68-72     optim.SGD(trainable_params, lr, momentum=0.9, nesterov=True)     (one group per parameter: utils/learning.py:24-34)
 *   train_manager_mm.py:284       optimizer.step()
 * over a TABLE of tensors, so that a step is three launches for the whole model and five parameter-sized streams (read g, p and the momentum
 * buffer, write p and the buffer) plus one read of g for the norm, where torch's single-tensor path (torch/optim/sgd.py: _single_tensor_sgd,
 * the only one open with a group per parameter) runs several launches per tensor and about fifteen streams.
 *
 * The table is a DEVICE array of n_tensors records; `table_host` is the host array it was uploaded from (pinned or not).  The library copies
 * nothing: table_host is read by the host code to validate the call BEFORE anything is enqueued or written -- n >= 0, chunk_begin the running
 * prefix, their total == n_chunks <= 2^31 - 1, and for the step a non-NULL param (and momentum, when momentum != 0) wherever grad is set;
 * AOC_ERR_INVALID_ARG otherwise.  It may be NULL (a table built on the device): then only the scalars are checked and the records are trusted.
 * A tensor is cut into chunks of AOC_MT_CHUNK floats counted from its FIRST ELEMENT; chunk_begin is the number of chunks of the tensors in
 * front (an empty tensor owns none); one workgroup of 256 threads takes one chunk and finds its tensor by a binary search over chunk_begin
 * (no host-built chunk map).  A record whose grad is NULL is skipped everywhere: its parameter and buffer are not touched, and it adds nothing
 * to the norm.  All pointers are class 4: every access goes through 4-byte-aligned vector types, a tensor may start at any float, and no
 * summation order depends on an address -- the norm's bits do not depend on any pointer's alignment.  fp32, no float atomics: equal buffers
 * give equal bits.
 */
#define AOC_MT_CHUNK 4096           /* floats per chunk: 16 per thread and stream, as four 16-byte accesses 4 KiB apart */
#define AOC_MT_HAS_MOMENTUM 1       /* aoc_mt_tensor.flags bit 0: the momentum buffer holds a value                   */
typedef struct aoc_mt_tensor {
    float *param;                    /* [n]; may be NULL for the norm, the scale and the zeroing */
    float *grad;                     /* [n] or NULL: the tensor has no gradient this step        */
    float *momentum;                 /* [n]; may be NULL when momentum == 0                      */
    int64_t n;
    int64_t chunk_begin;
    float weight_decay;
    int32_t flags;
} aoc_mt_tensor;
int64_t aoc_mt_chunks(int64_t n);   /* ceil(n / AOC_MT_CHUNK); 0 for n <= 0 */
/* aoc_grad_sumsq_partials: partial[c] (n_chunks doubles, 8-byte aligned) = the sum of g^2 over chunk c: thread t of 256 owns the floats
 * 1024 j + 4 t .. + 3 of the chunk (j = 0 .. 3) and adds their squares in ascending address in float32 from 0.0f, each square rounded before it
 * is added; then the xor butterfly over the wave (32 .. 1), then the four wave sums ascending ((w0 + w1) + w2) + w3; widened to double.  Floats
 * behind the tensor's end count as +0.0f; a chunk of a tensor without grad gives 0.0.  The first half of clip_grad_norm_ (norm_type 2). */
int aoc_grad_sumsq_partials(const aoc_mt_tensor *table, const aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, double *partial,
                            aoc_stream_t stream);
/* aoc_grad_norm_finish: one workgroup; thread t adds partial[t], partial[t + 256], ... ascending in double from 0.0, the xor butterfly
 * (32 .. 1) and the four wave sums ascending, all in double; total_norm[0] = (float)sqrt(sum); coef[0] = c > 1 ? 1 : c with
 * c = max_norm / (total_norm + 1e-6f) in float32 (torch/nn/utils/clip_grad.py: clip_coef and its clamp(max=1.0); a NaN stays a NaN).  Both are
 * device words, each optional (not both NULL); nothing synchronises.  n_chunks == 0 gives total_norm 0. */
int aoc_grad_norm_finish(const double *partial, int64_t n_chunks, float max_norm, float *total_norm, float *coef, aoc_stream_t stream);
/* aoc_multi_tensor_scale: g = g * coef[0] in place for every record with a grad: the second half of a stand-alone clip_grad_norm_
 * (train_manager_mm.py:283).  aoc_multi_tensor_zero: g = 0.0f likewise (optimizer.zero_grad(set_to_none=False) as one launch). */
int aoc_multi_tensor_scale(const aoc_mt_tensor *table, const aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, const float *coef,
                           aoc_stream_t stream);
int aoc_multi_tensor_zero(const aoc_mt_tensor *table, const aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, aoc_stream_t stream);
/* aoc_sgd_step: train_manager_mm.py:284 with the clip of :283 folded in.  Per element, in this order, each operation rounded once (nothing fuses):
 *   g' = g * coef[0]                                                     (coef == NULL: 1.0f)
 *   d  = (wd != 0) ? g' + wd * p : g'                                    wd = the record's weight_decay; the clip first, the decay second
 *   b' = (flags & 1) ? momentum * b + (1.0f - dampening) * d : d         (skipped when momentum == 0; 1.0f - dampening formed once in float32)
 *   v  = nesterov ? d + momentum * b' : b'                               (v = d when momentum == 0)
 *   p' = p + (-lr) * v                                                   lr = lr_dev[tensor] when lr_dev != NULL (n_tensors device floats), else `lr`
 * which is torch's _single_tensor_sgd behind clip_grad_norm_.  Writes p' and b'; g is read with the non-temporal load and is written only with
 * zero_grad != 0, as 0.0f (the clipped value is never written back).  After a step with momentum != 0 bit 0 of `flags` is set in every record
 * that had a grad and n > 0 -- in the device table by one small launch behind the step, and in table_host by the host code, so that the mirror
 * keeps describing the device table and nothing is uploaded again; once every such record carries the bit that launch is not made.
 * AOC_ERR_INVALID_ARG: momentum < 0 (or NaN), nesterov with momentum == 0 or dampening != 0 (torch's own rule), and the table checks above. */
int aoc_sgd_step(aoc_mt_tensor *table, aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, const float *coef, float lr, const float *lr_dev,
                 float momentum, float dampening, int nesterov, int zero_grad, aoc_stream_t stream);
/* aoc_clip_sgd_step: aoc_grad_sumsq_partials, aoc_grad_norm_finish and aoc_sgd_step as ONE call: exactly those launches, with the partial
 * sums and the coefficient in the caller's workspace (8-byte aligned; aoc_clip_sgd_step_workspace_bytes(n_chunks), else AOC_ERR_WORKSPACE), so
 * every output has the bits of the separate calls.  total_norm (a device word) is required.  Everything is validated before the first launch. */
size_t aoc_clip_sgd_step_workspace_bytes(int64_t n_chunks);
int aoc_clip_sgd_step(aoc_mt_tensor *table, aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, float max_norm, float *total_norm, float lr,
                      const float *lr_dev, float momentum, float dampening, int nesterov, int zero_grad, void *workspace, size_t workspace_bytes,
                      aoc_stream_t stream);

/*
 * The hand-over between two frames of a training step (csrc/train_step.hip; aoc_amd.train_step): what train_manager_mm.py:241-284 does with the
 * model's prediction,
 *   train_manager_mm.py:277       iou = pytorch_iou(all_pred.unsqueeze(1), curr_labels, obj_nums)        (utils/metric.py:3-34)
 *   train_manager_mm.py:281-282   running_losses[idx].update(loss.item() * seq_len); running_ious[idx].update(iou.item())   (utils/meters.py)
 *   train_manager_mm.py:258-259   prev_labels = all_pred.unsqueeze(1), shrunk by aocnet.py:134-135 interpolate(mode='nearest').int()
 * as one call per frame for the whole batch: two launches, nothing allocated, nothing synchronised, every argument validated before the
 * first launch (a rejected call enqueues and writes nothing).
 *
 * pred, gt [bs, H, W], each with its own dtype code (AOC_LABEL_I32 / _I64 / _F32: float32 maps of integers, as the loader's masks are).  A
 * value v names object o iff v == o as numbers: 255, negatives, ids above the sample's obj_num and non-integers match nothing.
 * obj_num_host [bs]: a HOST array, each 0 .. AOC_MAX_OBJECTS (negative: AOC_ERR_INVALID_ARG, larger: AOC_ERR_UNSUPPORTED).
 * mode AOC_IOU_PER_COLUMN is the reference AS IT IS CALLED: with [bs, 1, H, W] inputs metric.py's `== obj_ids` broadcasts to [1, n, H, W]
 * and .sum((1, 2)) runs over the objects and the rows, so a sample's value is the mean over the W columns x of (I[x] + eps) / (U[x] + eps),
 *   I[x] = #rows with pred == gt and the id in 1 .. n            U[x] = sum over the rows of [pred in 1..n] + [gt in 1..n] - [both and equal]
 * mode AOC_IOU_PER_OBJECT is the function as documented ([bs, h, w] inputs): the mean over the objects o = 1 .. n of (I[o] + eps) / (U[o] + eps),
 *   I[o] = #pixels with pred == gt == o      U[o] = #pred[o] + #gt[o] - I[o]
 * Arithmetic, so that a float32 restatement gives the same bits: the counts are integers (how they are gathered changes nothing); a ratio is
 * ((float)I + eps) / ((float)U + eps), one rounding per operation; a sample's mean over its n terms (W columns or obj_num objects): thread
 * t of 256 adds the terms t, t + 256, ... ascending from 0.0f, then the xor butterfly over the wave (32 .. 1) and the four wave sums as
 * (w0 + w1) + (w2 + w3), then the division by (float)n; the batch mean: the samples with obj_num > 0 in ascending order from 0.0f, divided by
 * their number, 1.0f when there is none (metric.py's `continue` and its torch.ones).  H * W <= 2^24 and bs * H * W < 2^31, beyond either
 * AOC_ERR_UNSUPPORTED (without reading a buffer).  No float atomics, no atomics on global memory: equal inputs give equal bits.
 *
 * Outputs, each optional (NULL: skipped), at least one; each has alone the bits it has with the others:
 *   iou             one float
 *   iou_per_sample  [bs]; 1.0f where obj_num == 0 (such samples are left out of the batch mean)
 *   counts          mode 0: [bs, W, 2] uint32 = I[x], U[x];   mode 1: [bs, AOC_MAX_OBJECTS, 3] uint32 = I[o], #pred[o], #gt[o] (0 behind obj_num)
 *   prev_small      [bs, small_h, small_w] int32: pred through torch's nearest rule, source row min((int)floorf((float)y * ((float)H /
 *                   (float)small_h)), H - 1) and the column likewise; an int64 value is narrowed, a float one goes through (int)v.  Needs
 *                   small_h, small_w >= 1; with prev_small alone gt, obj_num_host and the workspace may be NULL (one launch)
 *   meter           one record updated with iou and n = 1 as aoc_meters_update does (8-byte aligned)
 * All other pointers are class 4 (an int64 map too: sample 1 of an odd H * W starts off every wider grid) and no bit depends on where one
 * sits.  The workspace (class 4, aoc_frame_handover_workspace_bytes(bs, H, W), else AOC_ERR_WORKSPACE) may hold anything on entry.
 *
 * aoc_meter follows utils/meters.py AverageMeter.update(val, n): with x = (double)value[0] * scale (the reference's `loss.item() * seq_len`
 * in Python's double arithmetic), val = (float)x, sum += x * n, count += n, avg = (float)(sum / count); a zeroed record is a fresh meter.
 * aoc_meters_update: one launch for k <= AOC_METERS_PER_CALL updates (more: AOC_ERR_UNSUPPORTED) of distinct meters index_host[j] < n_meters
 * of the device array `meters`, each from its own device float word values_host[j] with scale_host[j] and n_host[j] >= 1 (all four HOST
 * arrays; a repeated index, a NULL word or n < 1: AOC_ERR_INVALID_ARG).  aoc_meters_reset: one launch zeroes the meters whose bit is set in
 * `mask` (n_meters <= 64; a bit at or above n_meters: AOC_ERR_INVALID_ARG).  Neither synchronises.
 */
#define AOC_LABEL_I32 0
#define AOC_LABEL_I64 1
#define AOC_LABEL_F32 2
#define AOC_IOU_PER_COLUMN 0
#define AOC_IOU_PER_OBJECT 1
#define AOC_METERS_PER_CALL 8
typedef struct aoc_meter {
    float val;
    float avg;
    double sum;
    int64_t count;
} aoc_meter;
size_t aoc_frame_handover_workspace_bytes(int bs, int H, int W);
int aoc_frame_handover(const void *pred, int pred_dtype, const void *gt, int gt_dtype, int bs, int H, int W, const int32_t *obj_num_host,
                       float epsilon, int mode, int small_h, int small_w, float *iou, float *iou_per_sample, uint32_t *counts, int32_t *prev_small,
                       aoc_meter *meter, void *workspace, size_t workspace_bytes, aoc_stream_t stream);
int aoc_meters_update(aoc_meter *meters, int n_meters, const int32_t *index_host, const float *const *values_host, const double *scale_host,
                      const int64_t *n_host, int k, aoc_stream_t stream);
int aoc_meters_reset(aoc_meter *meters, int n_meters, uint64_t mask, aoc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AOC_HIP_H */
