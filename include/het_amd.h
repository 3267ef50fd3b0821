/*
 * het_amd.h -- C ABI of libhet_amd.so: MI355X (gfx950) kernels for the
 * relational-GNN hot path of K-Wu/HET (segment GEMM, hetero edge-softmax,
 * gather-scatter aggregation; forward and backward).
 *
 * The reference exposes this path as torch custom ops registered with
 * TORCH_LIBRARY_FRAGMENT(torch_hrt, m) (a dispatcher boundary, not a C ABI:
 * the .inc.h files under hrt/include/DGLHackKernel/OpExport/).  Every entry point below is the
 * plain-pointer form of one of those ops: same name (prefixed het_), same
 * argument meaning, with each at::Tensor replaced by its device pointer and
 * sizes, and each torch::Dict<string, Tensor> flattened into named pointers.
 * het_amd/kernels.py re-registers the ops under torch.ops.torch_hrt.* on top of
 * this ABI; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions (as the reference, RGNNOps.inc.h:191-199, RGATOps.inc.h:35-48):
 *   - all pointers are DEVICE pointers to contiguous buffers on the current HIP
 *     device; floats are fp32, indices int64;
 *   - outputs are caller-allocated; "+=" in a comment means accumulated into,
 *     "=" means overwritten (no pre-zeroing needed);
 *   - launches go to `stream` (a hipStream_t; NULL = default stream), nothing
 *     synchronises the host, nothing allocates -- except het_grouping_create;
 *   - return value 0 = ok; otherwise an HET_ERR_* code, message in
 *     het_last_error() (thread-local).  Arguments are validated on the host
 *     before any launch (the reference only has compiled-out asserts).
 *
 * Paths in comments are relative to /root/reference/hrt/.
 */
#ifndef HET_AMD_H
#define HET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HET_OK 0
#define HET_ERR_INVALID_ARG 1
#define HET_ERR_HIP 2
#define HET_ERR_UNSUPPORTED 3

typedef void* het_stream; /* hipStream_t */
/* a bfloat16 value: the upper 16 bits of an IEEE float (the layer entries named *_bf16 take activation rows of it) */
typedef uint16_t het_bf16;

/* CompactAsOfNodeKind, include/kernel_enums.h:6-14 (the int the ops take) */
#define HET_KIND_DISABLED 0
#define HET_KIND_ENABLED 1
#define HET_KIND_DIRECT_INDEX 2
#define HET_KIND_DUAL_LIST 3
#define HET_KIND_DUAL_LIST_DIRECT_INDEX 4

/* replaces torch.ops.torch_hrt.build_debug_info (buildutils/genutils/gen_headers.py:17-41) */
const char* het_build_info(void);
const char* het_last_error(void);

/* Per-kernel device timing for bench.py's roofline figures (no reference counterpart: the reference times whole
 * forward / backward passes with CUDA events, RGNNUtils.py:291-311).  While enabled, the library records a HIP event
 * pair on the launch stream around every launch of its dominant kernels (the kernel alone, not the entry point's
 * fills or neighbouring launches).  het_kernel_timing_read synchronises the recorded events and returns the summed
 * duration and the number of launches of the kernels whose name starts with `name_prefix` (the __global__ name as
 * rocprofv3 prints it, without template arguments, e.g. "HET_gat_aggregate").  Enabling clears earlier records. */
int het_kernel_timing_enable(int on);
int het_kernel_timing_read(const char* name_prefix, double* total_ms, int64_t* launches);

/* ------------------------------------------------------------------------
 * Groupings: a one-time, device-side preprocessing of an index list that the
 * fast paths use to replace float atomics by segmented reductions.  A grouping
 * sorts the E positions of a relation-bucketed list by (relation, key[i]) --
 * or by key[i] alone when rel_ptrs is NULL -- and records the segments.  It has
 * no counterpart in the reference (which uses atomicAdd everywhere, e.g.
 * RGAT/RGATKernelsSeparateCOO.cu.h:77,195); every op accepts NULL instead and
 * then runs its atomics-based kernel.  Allocates device memory (hipMalloc, or
 * the caller's allocator: het_set_allocator) and synchronises `stream` once;
 * destroy with het_grouping_destroy.
 * ------------------------------------------------------------------------ */
/* Device memory the library keeps beyond a call (groupings, their lazily built lists) and its construction scratch comes
 * from hipMalloc / hipFree unless the host side installs its own allocator -- a framework binding passes its caching
 * allocator here (csrc/torch_export.cpp: c10::hip::HIPCachingAllocator; het_amd/_lib.py: torch.cuda.caching_allocator_alloc),
 * so that the groupings show up in that allocator's statistics, are returned to its pool when a cache evicts them, and no
 * hipFree (a device-wide synchronisation) happens on an op's path.  `stream`: the stream the memory is first used on.
 * alloc returns NULL on failure.  A pointer is always released through the allocator it came from, also after the
 * allocator was changed or reset (NULL, NULL: back to hipMalloc).  No counterpart in the reference (its launchers allocate
 * thrust::device_vector scratch per call, RGNNOps.inc.h:163-169). */
typedef void* (*het_alloc_fn)(size_t bytes, het_stream stream, void* user);
typedef void (*het_free_fn)(void* ptr, void* user);
int het_set_allocator(het_alloc_fn alloc, het_free_fn free_, void* user);
int het_allocator_is_external(void); /* 1 while an allocator is installed */
typedef struct het_grouping het_grouping;
/* payload0/payload1 (optional, [E]): per-position int64 arrays that are carried along in sorted
 * order (stored as int32), so that a grouped kernel reads them coalesced instead of chasing
 * perm -> array.  Each op documents what it expects there. */
int het_grouping_create(const int64_t* rel_ptrs /* [R+1] or NULL */, int64_t num_rels,
                        const int64_t* keys /* [E] */, int64_t num_positions, int64_t key_bound,
                        const int64_t* payload0, const int64_t* payload1,
                        het_stream stream, het_grouping** out);
void het_grouping_destroy(het_grouping* g);
/* Lifetime across streams.  All arrays of a grouping -- the lists the library builds on first use included -- belong to the
 * stream (and device) it was created on: a list first needed on another stream is allocated on the creation stream all the same,
 * and its build on that other stream is ordered after the creation stream's earlier work.  With the default allocator
 * het_grouping_destroy ends in hipFree, which waits for the device.  With a stream-ordered allocator installed
 * (het_set_allocator: torch's caching allocator in both torch registrations) a freed block is handed out again to that stream
 * at once, so a binding that runs ops with the grouping on ANOTHER stream reports that stream here (cheap; idempotent): destroy
 * then makes the creation stream wait for an event on every reported stream before it releases anything -- no host
 * synchronisation -- whichever device is current when it is called.  Both registrations call it on every cache lookup
 * (het_amd/plan.py, csrc/torch_export.cpp). */
void het_grouping_note_stream(const het_grouping* g, het_stream stream);
/* number of segments (distinct (relation, key) pairs) */
int64_t het_grouping_num_segments(const het_grouping* g);
/* device bytes the grouping currently holds: the sum of its allocations, the lists built on first use so far and the ones a
 * rebuild replaced included (with the default hipMalloc they are outside the caller's allocator statistics) */
int64_t het_grouping_bytes(const het_grouping* g);
/* out[i] = sorted rank of position i (the inverse of the grouping's permutation), [E] */
int het_grouping_rank_of_position(const het_grouping* g, int64_t* out, het_stream stream);
/* map[r, k] = segment of (relation r, key k) of a grouping by (relation, key), -1 where that pair has no position; map
 * [R, num_keys] int32, num_keys >= the grouping's key bound.  (Segments are in ascending (relation, key) order: segment s is
 * row s of the sorted unique (relation, key) list of the positions -- het_node_row_map on that list gives the same map.) */
int het_grouping_segment_map(const het_grouping* g, int64_t num_keys, int32_t* map, het_stream stream);
/* out[j, :] = values[payload1 of sorted rank j, :] (H floats per entry, [E, H]): per-edge-id values (an edge norm) brought into the
 * grouping's order once, for callers that pass the same values every step -- the passes then read them as a stream */
int het_grouping_gather_payload1(const het_grouping* g, const float* values, int64_t H, float* out, het_stream stream);

/* ------------------------------------------------------------------------
 * a1  rgnn_relational_matmul            OpExport/RGNNOps.inc.h:238-295
 *   kind 0: ret[scatter_idx[i], h, :] = x[gather_idx[i], (h), :] . W[r(i), h]    i in [0, num_rows)
 *           (dict keys separate_coo_rel_ptrs / separate_coo_node_indices / separate_coo_eids)
 *   kind 1: ret[i, h, :] = x[gather_idx[i], (h), :] . W[r(i), h]   scatter_idx = NULL
 *           (dict keys unique_srcs_and_dests_rel_ptrs / unique_srcs_and_dests_node_indices)
 *   W [R,H,K,D]; x [*, K] if in1head else [*, H, K]; ret [*, H, D].
 *   by_rel_gather (optional, kind 0: the grouping of a2 -- positions by (relation, gather_idx), payload0 =
 *   scatter_idx) + workspace of S*H floats: with in1head and D == 1 (RGAT's --multiply_among_weights_first_flag:
 *   er = x[dst] . (W.attn_r)) the S distinct (relation, x row) products are formed once and duplicated to their
 *   positions -- same values.  NULL / 0: every position is computed on its own.
 * ------------------------------------------------------------------------ */
int het_rgnn_relational_matmul(int64_t kind, const int64_t* rel_ptrs, int64_t num_rels,
                               const int64_t* gather_idx, const int64_t* scatter_idx, int64_t num_rows,
                               const float* weights, const float* x, float* ret,
                               int64_t H, int64_t K, int64_t D, int in1head,
                               const het_grouping* by_rel_gather, void* workspace, int64_t workspace_bytes,
                               het_stream stream);

/* a1 + the attention-vector product of RGAT in the GEMM epilogue (extension; RGAT/models.py:288-296 computes
 * el = <feat, attn_l[r]> with a second, D_out = 1 segment GEMM that re-reads the [rows,H,D] tensor just written):
 *   ret as het_rgnn_relational_matmul with in1head = 1, and
 *   dot_out[scatter_idx[i], h] = < ret[scatter_idx[i], h, :], dot_w[r, h, :] >       dot_w [R,H,D], dot_out [*,H]
 * MFMA shapes only (K and H*D in {32, 64, 128}, D a power of two >= 4): HET_ERR_UNSUPPORTED otherwise.
 * by_rel_gather (optional, kind 0; the grouping of a2) + workspace of S*(H*D + H) floats: rows that share
 * (relation, gather_idx) are identical, so the GEMM runs on the S distinct rows and a broadcast kernel duplicates
 * them to their positions (same values; on ogbn-mag S = 3.7 M of E = 21.1 M rows by source).
 * comp_rows (optional, [S, H*D]): receives the distinct rows (the workspace then needs S*H floats only).
 * ret == NULL (grouping path only, H a power of two >= 4): the caller wants dot_out alone -- RGAT's er, whose
 * per-edge projection no other op reads -- and the [E,H,D] tensor is never written.
 * dot_grouping (optional, grouping path only): a grouping of the same (relation, gather_idx) keys whose payload0 says
 * where the dots of every position go (dot_out[payload0[i], h]) when that is not scatter_idx -- e.g. the rank of the
 * edge in the destination-grouped order of a4, so that a4 reads el / er as coalesced streams. */
int het_rgnn_relational_matmul_attn_dot(int64_t kind, const int64_t* rel_ptrs, int64_t num_rels,
                                        const int64_t* gather_idx, const int64_t* scatter_idx, int64_t num_rows,
                                        const float* weights, const float* x, float* ret, const float* dot_w,
                                        float* dot_out, int64_t H, int64_t K, int64_t D,
                                        const het_grouping* by_rel_gather, void* workspace, int64_t workspace_bytes,
                                        float* comp_rows, const het_grouping* dot_grouping, het_stream stream);

/* backward of the above for a caller that used only dot_out (RGAT's er = <x[dst].W, attn_r>): the gradient of ret is
 * grad_dot (x) dot_w[r], rank one per head, so the (relation, gather_idx) segment sums are taken over the [rows,H]
 * gradient: gs = SUM grad_dot;  G = gs * dot_w[r];  grad_x[v] (+)= G . Wt[r];  grad_w[r] (+)= x[v]^T (x) G.
 * Needs by_rel_gather (as in a2) and a workspace of (S*H rounded up to 4) + S*H*D floats; HET_ERR_UNSUPPORTED otherwise.
 * The gradient of dot_w: with comp_rows (the distinct rows kept from the forward) and grad_dot_w [R,H,D] it is formed
 * here as SUM_s gs[s,h] * comp_rows[s,h,:]; otherwise it is the plain D_out = 1 weight gradient over the [E,H,D]
 * tensor (het_backward_rgnn_relational_matmul with grad_x = NULL). */
int het_backward_rgnn_relational_matmul_attn_dot_only(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx,
                                                      const int64_t* scatter_idx, int64_t num_rows, int64_t num_x_rows,
                                                      const float* weights_t, const float* x, const float* dot_w,
                                                      const float* grad_dot, float* grad_x, float* grad_w, int64_t H,
                                                      int64_t K, int64_t D, int accumulate,
                                                      const het_grouping* by_rel_gather, void* workspace,
                                                      int64_t workspace_bytes, const float* comp_rows,
                                                      float* grad_dot_w, het_stream stream);

/* a2  backward_rgnn_relational_matmul   OpExport/RGNNOps.inc.h:946-1010
 *   grad_x[gather_idx[i], (h), :] += gradout[scatter_idx[i], h, :] . Wt[r, h]   (heads summed iff in1head)
 *   grad_w[r, h]                  += x[gather_idx[i], (h), :]^T (x) gradout[scatter_idx[i], h, :]
 *   weights_t [R,H,D,K].  by_rel_gather: optional grouping of the rows by (relation, gather_idx):
 *   het_grouping_create(rel_ptrs, R, gather_idx, num_rows, <rows of x>, payload0 = scatter_idx, NULL, ...);
 *   with it, `workspace` must hold het_grouping_num_segments(g) * H * D floats (16-byte aligned).
 *   accumulate != 0: "+=" into the caller's buffers as the reference does (its wrapper zero-fills them,
 *   rgnn_layers_and_funcs.py:52-55); accumulate == 0: grad_x and grad_w are overwritten, no pre-zeroing
 *   needed (saves a fill + a read-modify-write pass when every grad_x row has a single writer).
 *   grad_x may be NULL for the D == 1 shapes (attention vectors, per-head or shared input): weight gradient only.
 *   `accumulate` is a bit set: HET_ACC_ADD (1) as above; HET_ACC_DISTINCT_ROWS (2), kind 1 only: the caller GUARANTEES
 *   that gather_idx holds a node at most once inside every relation (a unique (relation, node) list, what the reference's
 *   graph builders produce).  Only with that bit are the input gradients of a relation added with plain
 *   read-modify-write, relation by relation (deterministic, faster); without it -- the reference-named torch op -- any
 *   list is valid, duplicates included, and the adds are float atomics as in the reference's compact backward
 *   (RGNN/my_shmem_sgemm_func.cu.h:711-776).  A list with duplicates passed WITH the bit loses contributions. */
#define HET_ACC_ADD 1
#define HET_ACC_DISTINCT_ROWS 2
int het_backward_rgnn_relational_matmul(int64_t kind, const int64_t* rel_ptrs, int64_t num_rels,
                                        const int64_t* gather_idx, const int64_t* scatter_idx, int64_t num_rows,
                                        int64_t num_x_rows /* rows of x and grad_x */,
                                        const float* weights_t, const float* x, const float* gradout,
                                        float* grad_x, float* grad_w,
                                        int64_t H, int64_t K, int64_t D, int in1head, int accumulate,
                                        const het_grouping* by_rel_gather, void* workspace,
                                        int64_t workspace_bytes, het_stream stream);

/* a3  rgnn_relational_matmul_no_scatter_gather_list / backward_...   RGNNOps.inc.h:21-88, 660-753
 *   rows offsets[t]:offsets[t+1] use W[t]; x is [rows, K] (x_per_head = 0) or [rows, H, K]. */
int het_rgnn_relational_matmul_no_scatter_gather_list(const int64_t* offsets, int64_t num_types, int64_t num_rows,
                                                      const float* weights, const float* x, float* ret,
                                                      int64_t H, int64_t K, int64_t D, int x_per_head,
                                                      het_stream stream);
int het_backward_rgnn_relational_matmul_no_scatter_gather_list(const int64_t* offsets, int64_t num_types,
                                                               int64_t num_rows, const float* weights_t,
                                                               const float* x, const float* gradout,
                                                               float* grad_x, float* grad_w,
                                                               int64_t H, int64_t K, int64_t D, int x_per_head,
                                                               int accumulate, het_stream stream);

/* ------------------------------------------------------------------------
 * a4  relational_fused_gat_separate_coo    OpExport/RGATOps.inc.h:170-245
 *   exp[eids[i], h]  = leaky_exp(el[srow(i), h] + er[drow(i), h])
 *   sum[col[i], h]   = SUM_i exp            (all in-edges of the destination, every relation)
 *   ret[col[i],h,:]  = SUM_i exp/sum * feat[srow(i), h, :]
 *   sum, exp, ret are overwritten (zeroed internally; the reference accumulates into
 *   uninitialised buffers).
 * Row maps by kind (dict of the reference op flattened into four pointers):
 *   kind 0  srow = drow = eids[i]                               all four NULL
 *   kind 1  srow/drow = row of (r(i), row[i]) / (r(i), col[i]) in the unique list
 *           map_row_a = map_col_a = unique_srcs_and_dests_rel_ptrs [R+1]
 *           map_row_b = map_col_b = unique_srcs_and_dests_node_indices
 *   kind 3  map_row_a/b = unique_srcs_and_dests_rel_ptrs / ..._node_indices_row
 *           map_col_a/b = unique_srcs_and_dests_rel_ptrs_col / ..._node_indices_col
 *   kind 4  srow = map_row_a[eids[i]], drow = map_col_a[eids[i]]
 *           (edata_idx_to_inverse_idx_row / _col); map_*_b NULL
 *   feat [n_src_rows, H, D]; el [n_src_rows, H]; er [n_dst_rows, H]; sum [N,H]; exp [E,H]; ret [N,H,D].
 *   by_dst: optional grouping of the positions by col: het_grouping_create(NULL, 0, col, E, N,
 *   payload0 = eids, payload1 = NULL or the feat row of every position (srow), ...).
 *   exp_sorted (optional, [E,H], needs by_dst): a second copy of exp in the grouping's order, which the
 *   backward can stream instead of gathering exp / el / er by edge id.
 *   el_sorted, er_sorted (extension, kind 0 with by_dst and exp_sorted; both or neither): [E,H], the attention terms
 *   already in the grouping's order (row j = the edge at sorted rank j, het_grouping_rank_of_position).  The
 *   aggregation pass then forms exp itself from two coalesced streams -- no separate exp pass, no per-edge 16-byte
 *   gathers -- and writes exp_sorted; el, er may be NULL, exp (edge order) is written only if not NULL.
 * ------------------------------------------------------------------------ */
int het_relational_fused_gat_separate_coo(const int64_t* eids, const int64_t* rel_ptrs, const int64_t* row,
                                          const int64_t* col, int64_t num_rels, int64_t num_edges,
                                          int64_t num_nodes, int64_t kind,
                                          const int64_t* map_row_a, const int64_t* map_row_b,
                                          const int64_t* map_col_a, const int64_t* map_col_b,
                                          const float* feat, const float* el, const float* er,
                                          float* sum, float* exp, float* ret, float* exp_sorted,
                                          int64_t H, int64_t D, double slope,
                                          const het_grouping* by_dst, const float* el_sorted, const float* er_sorted,
                                          het_stream stream);

/* a5  backward_relational_fused_gat_separate_coo   OpExport/RGATOps.inc.h:465-551
 *   a = exp[eids[i],h] / sum[col[i],h]
 *   grad_feat[srow,h,:] += a * gradout[col[i],h,:]
 *   t = SUM_d gradout[col[i],h,d] * (feat[srow,h,d] - ret[col[i],h,d]) * a * (z > 0 ? 1 : slope)
 *   grad_el[srow,h] += t ; grad_er[drow,h] += t
 *   kind 0: every feat/el/er row belongs to one edge, so the three gradients are OVERWRITTEN (stores, no
 *   atomics, no pre-zeroing needed) and grad_er may alias grad_el (same values).  Other kinds: "+=".
 *   exp_sorted: optional copy of exp in by_dst order written by the forward (slope >= 0 required: the
 *   leaky-ReLU branch is then recovered from exp > 1); with it (kind 0, by_dst) el, er and exp are not read and
 *   may be NULL.
 *   Compact kinds, optional fast path (slope >= 0): by_src_row = het_grouping_create(NULL, 0, srow, E,
 *   n_src_rows, payload0 = eids, payload1 = col) over the feat row of every position, by_dst_row likewise
 *   over the er row (payload0 = eids), workspace of (N*2H + E*H) floats; grad_feat / grad_el / grad_er are
 *   then overwritten.  n_src_rows / n_dst_rows: rows of feat/el and of er.
 *   fold_attn_l (extension, NULL = the reference op): [R,H,D]; for a caller that formed
 *   el[e,h] = <feat[e,h,:], fold_attn_l[r,h,:]> (RGAT/models.py:288-296) the gradient through that product,
 *   grad_el[e,h] * fold_attn_l[r,h,:], is added into grad_feat by the same store -- kind 0 with by_dst only
 *   (error otherwise; by_dst must then carry payload1 = relation of every position); replaces a
 *   read-modify-write pass over the [E,H,D] gradient.  grad_fold_attn_l (optional with fold_attn_l, R <= 8): [R,H,D],
 *   receives += SUM_e grad_el[e,h] * feat[e,h,:] per relation -- the weight gradient of that product, from the feat
 *   rows the kernel reads anyway (saves a pass over feat); the caller zero-fills it.  With a workspace of
 *   64*R*H*D floats (kind 0) the workgroups spread their final atomic adds over 64 copies that a last tiny kernel
 *   sums -- on small graphs all workgroups finish together and would serialise on the R*H*D words.
 *   Compact kinds with the by_src_row / by_dst_row groupings: fold_attn_l works on the compact rows
 *   (el[u,h] = <feat[u,h,:], fold_attn_l[r(u),h,:]>), fold_row_rel_ptrs [R+1] = the rows' relation pointers.
 *   grad_el_sorted (extension, kind 0 with by_dst only): [E,H], receives grad_el in by_dst order (row j = the edge at
 *   sorted rank j, see het_grouping_rank_of_position) -- sequential 16-byte stores instead of scattered ones, and a
 *   consumer that sums it by (relation, destination) reads contiguous runs.  grad_el / grad_er may then be NULL. */
int het_backward_relational_fused_gat_separate_coo(const int64_t* eids, const int64_t* rel_ptrs,
                                                   const int64_t* row, const int64_t* col, int64_t num_rels,
                                                   int64_t num_edges, int64_t num_nodes, int64_t kind,
                                                   const int64_t* map_row_a, const int64_t* map_row_b,
                                                   const int64_t* map_col_a, const int64_t* map_col_b,
                                                   const float* feat, const float* el, const float* er,
                                                   const float* sum, const float* exp, const float* ret,
                                                   const float* exp_sorted,
                                                   const float* gradout, float* grad_feat, float* grad_el,
                                                   float* grad_er, int64_t H, int64_t D, double slope,
                                                   const het_grouping* by_dst, const het_grouping* by_src_row,
                                                   const het_grouping* by_dst_row, int64_t n_src_rows,
                                                   int64_t n_dst_rows, void* workspace, int64_t workspace_bytes,
                                                   const float* fold_attn_l, float* grad_fold_attn_l,
                                                   const int64_t* fold_row_rel_ptrs, float* grad_el_sorted,
                                                   het_stream stream);

/* a6  relational_fused_gat_csr / backward_relational_fused_gat_csr   RGATOps.inc.h:251-277, 430-460
 *   forward over the in-CSR (rows = dst, col_indices = src); backward over the out-CSR
 *   (rows = src, col_indices = dst).  compact != 0: feat/el/er rows are (relation, node) rows of
 *   the unique list (uniq_rel_ptrs, uniq_node_idx), binary-searched. */
int het_relational_fused_gat_csr(const int64_t* in_row_ptrs, const int64_t* in_col, const int64_t* in_eids,
                                 const int64_t* in_reltypes, int64_t num_nodes, int64_t num_edges,
                                 const int64_t* uniq_rel_ptrs, const int64_t* uniq_node_idx, int64_t num_rels,
                                 const float* feat, const float* el, const float* er,
                                 float* sum, float* exp, float* ret, int64_t H, int64_t D, double slope,
                                 int compact, het_stream stream);
int het_backward_relational_fused_gat_csr(const int64_t* out_row_ptrs, const int64_t* out_col,
                                          const int64_t* out_eids, const int64_t* out_reltypes,
                                          int64_t num_nodes, int64_t num_edges,
                                          const int64_t* uniq_rel_ptrs, const int64_t* uniq_node_idx,
                                          int64_t num_rels, const float* feat, const float* el, const float* er,
                                          const float* sum, const float* exp, const float* ret,
                                          const float* gradout, float* grad_feat, float* grad_el, float* grad_er,
                                          int64_t H, int64_t D, double slope, int compact, het_stream stream);

/* ------------------------------------------------------------------------
 * a7  rgcn_layer1_separate_coo            OpExport/RGCNOps.inc.h:84-138
 *   ret[col[i], :] += (x[row[i], :] * norm[eids[i]]) . W[r(i)]        W [R,K,D]
 *   by_rel_dst: optional grouping of the positions by (relation, col):
 *   het_grouping_create(rel_ptrs, R, col, E, N, payload0 = row, payload1 = eids, ...) with a workspace of
 *   het_grouping_num_segments(g) * K floats; the backward takes the grouping by (relation, row) with
 *   payload0 = col, payload1 = eids and num_segments * D floats.
 * a8  backward_rgcn_layer1_separate_coo   OpExport/RGCNOps.inc.h:368-467
 *   grad_x[row[i], :] += (gradout[col[i], :] * norm[eids[i]]) . Wt[r]   (intended direction)
 *   grad_w[r]         += (x[row[i], :] * norm[eids[i]])^T (x) gradout[col[i], :]
 *   grad_norm is not written (disabled in the reference, my_shmem_sgemm_func_rgcn_hgt.cu.h:680-684).
 * ------------------------------------------------------------------------ */
int het_rgcn_layer1_separate_coo(const int64_t* rel_ptrs, const int64_t* eids, const int64_t* row,
                                 const int64_t* col, int64_t num_rels, int64_t num_edges, int64_t num_nodes,
                                 const float* x, const float* weights, const float* norm, float* ret,
                                 int64_t K, int64_t D, const het_grouping* by_rel_dst, void* workspace,
                                 int64_t workspace_bytes, het_stream stream);
int het_backward_rgcn_layer1_separate_coo(const int64_t* rel_ptrs, const int64_t* eids, const int64_t* row,
                                          const int64_t* col, int64_t num_rels, int64_t num_edges,
                                          int64_t num_nodes, const float* x, const float* weights_t,
                                          const float* norm, float* grad_norm, float* grad_x,
                                          const float* gradout, float* grad_w, int64_t K, int64_t D,
                                          const het_grouping* by_rel_src, void* workspace, int64_t workspace_bytes,
                                          het_stream stream);

/* a9  rgcn_node_mean_aggregation_compact_as_of_node_separate_coo (+ backward)  RGCNOps.inc.h:24-82, 303-366
 *   ret[col[i], :]        = SUM_i enorm[eids[i]] * feat[crow(i), :]            (ret overwritten)
 *   grad_feat[crow(i), :] += enorm[eids[i]] * gradout[col[i], :]
 *   crow(i) = map_a[eids[i]] if direct (inverse_indices_row), else the row of (r(i), row[i]) in the
 *   unique list map_a = rel_ptrs_row [R+1], map_b = node_indices_row  (intended mapping).
 *   Optional fast paths (X a power of two in 4..256): by_dst = het_grouping_create(NULL, 0, col, E, N, payload0 = crow
 *   per position, payload1 = eids); by_src_row = het_grouping_create(NULL, 0, crow, E, n_src_rows, payload0 = col,
 *   payload1 = eids): segmented sums instead of E*X float atomics. */
int het_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(
    const int64_t* eids, const int64_t* rel_ptrs, const int64_t* row, const int64_t* col, int64_t num_rels,
    int64_t num_edges, int64_t num_nodes, const int64_t* map_a, const int64_t* map_b, const float* feat,
    const float* enorm, float* ret, int64_t X, int direct, const het_grouping* by_dst, het_stream stream);
int het_backward_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(
    const int64_t* eids, const int64_t* rel_ptrs, const int64_t* row, const int64_t* col, int64_t num_rels,
    int64_t num_edges, int64_t num_nodes, const int64_t* map_a, const int64_t* map_b, const float* feat,
    const float* enorm, const float* ret, const float* gradout, float* grad_feat, int64_t X, int direct,
    const het_grouping* by_src_row, int64_t n_src_rows, het_stream stream);

/* ------------------------------------------------------------------------
 * a10  hgt_full_graph_edge_softmax_ops_separate_coo     OpExport/HGTOpsEdgeParallel.inc.h:18-31 -> HGTOps.inc.h:23-106
 *   m[eids[i],h] = exp(score[eids[i],h] * mu[r(i),h]);  sum[col[i],h] = SUM_i m;  a = m / sum[col[i],h]
 *   (denominator keyed by the DESTINATION over all E edges: intended semantics).
 *   sum, m, a are overwritten.
 *      backward_hgt_full_graph_enorm_to_unnormalized_attn_score_separate_coo   HGTOps.inc.h:597-648
 *   tmp[col[i],h] = SUM_i a*grad_a;  c = (grad_a - tmp[col[i],h]) * a
 *   grad_score[eids[i],h] = c * mu[r,h];  grad_mu[r,h] += c * score[eids[i],h]      
 *   by_dst (optional, H % 4 == 0): het_grouping_create(NULL, 0, col, E, N, payload0 = eids, payload1 = relation of
 *   every position) -- the denominators / tmp become segmented sums instead of E*H float atomics.
 * ------------------------------------------------------------------------ */
int het_hgt_full_graph_edge_softmax_ops_separate_coo(const int64_t* row, const int64_t* col, const int64_t* eids,
                                                     const int64_t* rel_ptrs, int64_t num_rels, int64_t num_edges,
                                                     int64_t num_nodes, const float* score, const float* mu,
                                                     float* sum, float* m, float* a, int64_t H,
                                                     const het_grouping* by_dst, het_stream stream);
int het_backward_hgt_full_graph_enorm_to_unnormalized_attn_score_separate_coo(
    const int64_t* row, const int64_t* col, const int64_t* eids, const int64_t* rel_ptrs, int64_t num_rels,
    int64_t num_edges, int64_t num_nodes, const float* score, const float* a, const float* grad_a, const float* mu,
    float* grad_score, float* grad_mu, float* tmp, int64_t H, const het_grouping* by_dst, het_stream stream);

/* a10c HGT's unfused aggregation on the CSR layouts (hgt_layers_and_funcs.py:298-422, the path of
 *      --fused_message_mean_aggregation_flag off).  The same formulas as a10 with the edges given as a CSR:
 *      row_ptrs [num_nodes + 1] (row_ptrs_len is its length and must equal num_nodes + 1), col_indices / eids /
 *      reltypes [num_edges] per position.  In-CSR rows are destinations (col = source); out-CSR rows are sources
 *      (col = destination).  Score tensors are [E,H] rows indexed by eids[i]; message rows are [E,H,dk]; node rows
 *      ([N,H] sums, [N,H,dk] out / gradout / ret) by node id.  r(i) = reltypes[i], v(i) = the destination of position i.
 *      by_dst (optional): het_grouping_create(NULL, 0, <destination of every position>, E, N, payload0 = eids,
 *      payload1 = reltypes) -- the in-CSR's expanded rows, or the out-CSR's col_indices.  With it (and H % 4 == 0 for
 *      the score-only ops, dk a power of two >= 4 with 8 <= H*dk <= 256 for the message ops, 16-byte aligned rows) a
 *      wave per work item reduces a destination in registers; destinations with more than HET_ITEM_MAX in-edges are
 *      split over several items whose partial sums meet in float atomics.  Otherwise a plain thread-per-element kernel
 *      runs.  Host-side checks (HET_ERR_INVALID_ARG before any launch): sizes, row_ptrs_len, null pointers.
 *
 *      hgt_full_graph_edge_softmax_ops_csr                 HGTOps.inc.h:190-204 -> 23-106 (switch 3, in-CSR)
 *   m[eids[i],h] = exp(mu[r(i),h] * score[eids[i],h]);  sum[v,h] = SUM over the in-edges of v of m;  a = m / sum[v,h]
 *   (no max subtraction: DESIGN.md Q2).  sum, m, a are overwritten (sum = 0 for a destination without in-edges).
 */
int het_hgt_full_graph_edge_softmax_ops_csr(const int64_t* row_ptrs, int64_t row_ptrs_len, const int64_t* col_indices,
                                            const int64_t* eids, const int64_t* reltypes, int64_t num_nodes,
                                            int64_t num_edges, const float* score, const float* mu, float* sum, float* m,
                                            float* a, int64_t H, const het_grouping* by_dst, het_stream stream);
/*      hgt_full_graph_message_mean_aggregation_csr         HGTOps.inc.h:180-188 -> 109-178 (switch 1, in-CSR)
 *   ret[v,h,:] = SUM over the in-edges of v of edge_attn_score[eids[i],h] / sum[v,h] * edge_messages[eids[i],h,:]
 *   edge_attn_score is the mu-applied UNNORMALISED score (m of the softmax); mu is not read.
 *   ret is overwritten (0 for a destination without in-edges). */
int het_hgt_full_graph_message_mean_aggregation_csr(const int64_t* row_ptrs, int64_t row_ptrs_len, const int64_t* col_indices,
                                                    const int64_t* reltypes, const int64_t* eids, int64_t num_nodes,
                                                    int64_t num_edges, const float* edge_messages,
                                                    const float* edge_attn_score, const float* sum, const float* mu,
                                                    float* ret, int64_t H, int64_t dk, const het_grouping* by_dst,
                                                    het_stream stream);
/*      backward_hgt_full_graph_message_mean_aggregation_csr   HGTOps.inc.h:477-487 -> 410-475 (switch 2, out-CSR)
 *   grad_message[eids[i],h,:] = a[eids[i],h] * gradout[col[i],h,:]     (every edge row written once: overwritten)
 *   sum is not read (the normalised score a is given).  No grouping: a map over the positions. */
int het_backward_hgt_full_graph_message_mean_aggregation_csr(const int64_t* row_ptrs, int64_t row_ptrs_len,
                                                             const int64_t* col_indices, const int64_t* reltypes,
                                                             const int64_t* eids, int64_t num_nodes, int64_t num_edges,
                                                             const float* sum, const float* normalized_attn_score,
                                                             const float* gradout, float* grad_message, int64_t H,
                                                             int64_t dk, het_stream stream);
/*      backward_hgt_full_graph_edge_softmax_ops_csr        HGTOps.inc.h:553-566 -> 489-551 (switch 2, out-CSR)
 *   c = a[eids[i],h] * < gradout[v,h,:], message[eids[i],h,:] - out[v,h,:] >       (v = col[i], per head)
 *   grad_attn_score[eids[i],h] = mu[r(i),h] * c    (overwritten)
 *   grad_mu[r(i),h] += c * score[eids[i],h]         (accumulated; every edge credits its own relation: DESIGN.md Q13)
 *   by_dst here groups the out-CSR positions by col_indices: a work item reads gradout[v] / out[v] once; grad_mu is
 *   reduced per block in LDS (num_rels * H <= 4096) and flushed with one atomic per (relation, head) and block. */
int het_backward_hgt_full_graph_edge_softmax_ops_csr(const int64_t* row_ptrs, int64_t row_ptrs_len, const int64_t* col_indices,
                                                     const int64_t* eids, const int64_t* reltypes, int64_t num_nodes,
                                                     int64_t num_edges, int64_t num_rels, const float* message,
                                                     const float* score, const float* normalized_attn_score,
                                                     const float* out, const float* gradout, const float* mu,
                                                     float* grad_attn_score, float* grad_mu, int64_t H, int64_t dk,
                                                     const het_grouping* by_dst, het_stream stream);
/*      backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr   HGTOps.inc.h:282-325 (in-CSR)
 *   the formulas of a10's backward:  tmp[v,h] = SUM over the in-edges of v of a*grad_a;  c = (grad_a - tmp[v,h]) * a
 *   grad_score[eids[i],h] = c * mu[r(i),h]   (overwritten);   grad_mu[r(i),h] += c * score[eids[i],h]   (accumulated)
 *   tmp stays in registers per destination; with by_dst and split hub destinations it is summed in `workspace`
 *   (num_nodes * H floats, 16-byte aligned); without room there the plain kernel runs. */
int het_backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr(
    const int64_t* row_ptrs, int64_t row_ptrs_len, const int64_t* col_indices, const int64_t* eids, const int64_t* reltypes,
    int64_t num_nodes, int64_t num_edges, int64_t num_rels, const float* score, const float* normalized_attn_score,
    const float* grad_normalized_attn_score, const float* mu, float* grad_score, float* grad_mu, int64_t H,
    const het_grouping* by_dst, void* workspace, int64_t workspace_bytes, het_stream stream);

/* a11  hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo (+ backward)
 *      OpExport/HGTOpsEdgeParallel.inc.h:33-88, 295-369
 *   new_h[col[i],h,:] += (v[row[i],h,:] * a[eids[i],h]) . W[r,h]                      W [R,H,dk,dout]
 *   grad_v[row[i],h,:] += (gradout[col[i],h,:] * a) . Wt[r,h]     (intended direction)
 *   grad_w[r,h]        += (v[row[i],h,:] * a)^T (x) gradout[col[i],h,:]
 *   grad_a[eids[i],h]   = < gradout[col[i],h,:] . Wt[r,h], v[row[i],h,:] >            Wt [R,H,dout,dk]
 *   Optional fast paths: by_rel_dst / by_rel_src are the groupings of rgcn_layer1 (by (relation, col) with
 *   payload0 = row, payload1 = eids; by (relation, row) with payload0 = col, payload1 = eids) and a workspace of
 *   num_segments * H * dk (forward) / num_segments * H * dout (backward) floats; heads wider than 16 floats
 *   (dk = dout = 32, 64, 128: the reference sweep's --num_heads 1) need 2 * num_segments * H * dout + R*H*dk*dout
 *   in the backward (grad_a is then taken from the per-(relation, source) message rows). */
int het_hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo(
    const int64_t* rel_ptrs, const int64_t* eids, const int64_t* row, const int64_t* col, int64_t num_rels,
    int64_t num_edges, int64_t num_nodes, const float* v, const float* weights, const float* a, float* new_h,
    int64_t H, int64_t dk, int64_t dout, const het_grouping* by_rel_dst, void* workspace, int64_t workspace_bytes,
    het_stream stream);
int het_backward_hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo(
    const int64_t* rel_ptrs, const int64_t* eids, const int64_t* row, const int64_t* col, int64_t num_rels,
    int64_t num_edges, int64_t num_nodes, const float* v, const float* weights_t, const float* a, const float* new_h,
    float* grad_v, float* grad_w, float* grad_a, const float* gradout, int64_t H, int64_t dk, int64_t dout,
    const het_grouping* by_rel_src, void* workspace, int64_t workspace_bytes, het_stream stream);

/* a12  rgnn_inner_product_right_node_separatecoo (+ backward)    OpExport/RGNNOps.inc.h:609-658, 1131-1181
 *   out[eids[i],h] = < left[lrow(i),h,:], right[row[i],h,:] >                               (out overwritten)
 *   lrow(i) = eids[i] (kind 0) | row of (r(i), col[i]) in the unique list map_a = rel_ptrs, map_b = node ids
 *             (kind 1) | map_a[eids[i]] (kind 2, edata_idx_to_inverse_idx)
 *   grad_left[lrow(i),h,:] += gradout[eids[i],h] * right[row[i],h,:];   grad_right[row[i],h,:] += ... * left[lrow(i),h,:]
 *   (accumulating; the reference kernel stores without atomics).  accumulate == 0: both
 *   gradients are overwritten instead (n_left_rows / n_right_rows = their row counts).  by_right: optional
 *   grouping of the positions by row (het_grouping_create(NULL, 0, row, E, n_right_rows, payload0 = lrow per
 *   position, payload1 = eids)), used for kinds 0 and 2.  by_left (kind 2): grouping of the positions by lrow
 *   (payload0 = row, payload1 = eids): the gradient of a shared compact row becomes a segmented sum instead of
 *   float atomics.  (A caller holding kind-1 lists can precompute lrow per edge id once and call with kind 2.) */
int het_rgnn_inner_product_right_node_separatecoo(int64_t kind, const int64_t* map_a, const int64_t* map_b,
                                                  const int64_t* rel_ptrs, const int64_t* eids, const int64_t* row,
                                                  const int64_t* col, int64_t num_rels, int64_t num_edges,
                                                  const float* left, const float* right, float* out, int64_t H,
                                                  int64_t D, het_stream stream);
int het_backward_inner_product_right_node_separatecoo(int64_t kind, const int64_t* map_a, const int64_t* map_b,
                                                      const int64_t* rel_ptrs, const int64_t* eids,
                                                      const int64_t* row, const int64_t* col, int64_t num_rels,
                                                      int64_t num_edges, const float* left, const float* right,
                                                      const float* gradout, float* grad_left, float* grad_right,
                                                      int64_t H, int64_t D, int accumulate,
                                                      const het_grouping* by_right, const het_grouping* by_left,
                                                      int64_t n_left_rows, int64_t n_right_rows, het_stream stream);

/*      hgt_full_graph_hetero_attention_ops_coo (+ backward)     OpExport/HGTOpsEdgeParallel.inc.h:95-158, 166-293
 *   inner[eids[i],h,:] = k[row[i],h,:] . W[r,h];   score[eids[i],h] = < inner[eids[i],h,:], q[col[i],h,:] >
 *   grad_q[col[i],h,:] += gs * inner[eids[i],h,:];  grad_k[row[i],h,:] += (gs * q[col[i],h,:]) . Wt[r,h];
 *   grad_w[r,h] += k[row[i],h,:]^T (x) (gs * q[col[i],h,:]),   gs = grad_score[eids[i],h]
 *   Optional fast path: by_dst (by col, payload0 = eids), by_rel_src (by (relation, row), payload0 = col,
 *   payload1 = eids), n_q_rows rows of q, workspace of by_rel_src segments * H * dout floats. */
int het_hgt_full_graph_hetero_attention_ops_coo(const int64_t* row, const int64_t* col, const int64_t* eids,
                                                const int64_t* rel_ptrs, int64_t num_rels, int64_t num_edges,
                                                const float* k, const float* q, const float* weights, float* inner,
                                                float* score, int64_t H, int64_t dk, int64_t dout, het_stream stream);
int het_backward_hgt_full_graph_hetero_attention_ops_coo(const int64_t* row, const int64_t* col, const int64_t* eids,
                                                         const int64_t* rel_ptrs, int64_t num_rels, int64_t num_edges,
                                                         float* grad_w, const float* weights_t, const float* k,
                                                         const float* q, const float* inner, const float* grad_score,
                                                         float* grad_k, float* grad_q, int64_t H, int64_t dk,
                                                         int64_t dout, const het_grouping* by_dst,
                                                         const het_grouping* by_rel_src, int64_t n_q_rows,
                                                         void* workspace, int64_t workspace_bytes, het_stream stream);

/* ------------------------------------------------------------------------
 * HGT attention + message aggregation on the distinct (relation, source) rows, without a per-edge float tensor
 * (layer-level fusion; no reference op of its own).  Inside the one-node HGT layer it replaces the chain
 * rgnn_relational_matmul (relation_att) -> rgnn_inner_product_right_node -> hgt_full_graph_edge_softmax_ops ->
 * hgt_full_graph_fused_message_calc_and_mean_aggregation and their backward ops (HGT/models.py:172-262;
 * OpExport/HGTOps.inc.h, OpExport/HGTOpsEdgeParallel.inc.h; kernels hrt/include/DGLHackKernel/HGT/ *.cu.h): same values,
 *   a_e[h] = exp(s_e[h]) / SUM_{e' into dst_e} exp(s_e'[h]),  s_e[h] = <k'[srow_e,h,:], q[dst_e,h,:]>,
 *   out[v,h,:] = SUM_{e into v} a_e[h] * m[srow_e,h,:]
 * with k' = k . relation_att . (relation_pri / sqrt(dk)) and m = v . relation_msg formed per distinct (relation, source)
 * row by the caller (one segment GEMM from the layer input when the typed projections are folded into the weights).
 *   kv_c [S_row, 2, H, D]: k' then m of every (relation, source) row;  q [N,H,D];  out [N,H,D];
 *   lsum [N,H] = log SUM exp(s) (the softmax subtracts a running maximum: finite for any score, unlike the reference's raw exp)
 *   by_dst:  het_grouping_create(NULL, 0, col, E, N, payload0 = (relation, source) row of every position, NULL)
 *   by_srow: het_grouping_create(NULL, 0, that row of every position, E, S_row, payload0 = col, NULL)
 * forward overwrites lsum and out (zero rows for destinations without in-edges); backward overwrites grad_kv_c [S_row,2,H,D]
 * and grad_q [N,H,D].  workspace (backward): het_hgt_backward_compact_workspace(N, H) bytes, 16-byte aligned; (forward):
 * het_hgt_aggregate_compact_workspace(by_dst, H, D) bytes (0 unless a destination has more than 256 in-edges).
 * Shapes: H*D in {8, 16, 32, 64, 128}, D a power of two >= 8 (het_hgt_compact_shape_ok); else HET_ERR_UNSUPPORTED.
 * The row tensors (kv_c, q, out, gradout, grad_kv_c, grad_q) must be 16-byte aligned: the kernels move them in 16-byte (fp32) or
 * 8-byte (bf16) pieces; a misaligned pointer is refused with HET_ERR_INVALID_ARG before anything is enqueued. */
int het_hgt_compact_shape_ok(int64_t H, int64_t D);
int het_hgt_aggregate_compact(const het_grouping* by_dst, const float* kv_c, const float* q, float* lsum, float* out,
                              int64_t num_nodes, int64_t num_src_rows, int64_t H, int64_t D, void* workspace,
                              int64_t workspace_bytes, het_stream stream);
int64_t het_hgt_aggregate_compact_workspace(const het_grouping* by_dst, int64_t H, int64_t D);
int64_t het_hgt_backward_compact_workspace(int64_t num_nodes, int64_t H);
int het_hgt_backward_compact(const het_grouping* by_dst, const het_grouping* by_srow, const float* kv_c, const float* q,
                             const float* lsum, const float* out, const float* gradout, float* grad_kv_c, float* grad_q,
                             int64_t num_nodes, int64_t num_src_rows, int64_t H, int64_t D, void* workspace,
                             int64_t workspace_bytes, het_stream stream);

/* The same pair with bf16 activation rows: kv_c, q, out and gradout are het_bf16 (the rows gathered once per edge: half the bytes);
 * lsum, grad_kv_c, grad_q, the workspaces and every sum, exponential and dot product are fp32 on widened values.  out is rounded
 * once (to nearest even) from acc / sum, for whole destinations and for hubs alike; the backward takes <gradout, out> from that
 * rounded out.  Arguments, validation, workspace queries and shapes are those of the fp32 pair. */
int het_hgt_aggregate_compact_bf16(const het_grouping* by_dst, const het_bf16* kv_c, const het_bf16* q, float* lsum, het_bf16* out,
                                   int64_t num_nodes, int64_t num_src_rows, int64_t H, int64_t D, void* workspace,
                                   int64_t workspace_bytes, het_stream stream);
int het_hgt_backward_compact_bf16(const het_grouping* by_dst, const het_grouping* by_srow, const het_bf16* kv_c, const het_bf16* q,
                                  const float* lsum, const het_bf16* out, const het_bf16* gradout, float* grad_kv_c, float* grad_q,
                                  int64_t num_nodes, int64_t num_src_rows, int64_t H, int64_t D, void* workspace,
                                  int64_t workspace_bytes, het_stream stream);

/* The per-step folding of the HGT layer's parameters into one source-side weight per relation (round 5; extension, reached from
 * het_amd/backend/hgt_fused_layer.py only), forward and backward as one / two launches instead of ~14 + ~24 torch kernels:
 *   w_kv[r, i, h*dk+e]         = pri[r,h] / sqrt(dk) * SUM_d k_lin[st(r), i, h*dk+d] * A[r,h,d,e]
 *   w_kv[r, i, H*dk + h*dk+e]  =                      SUM_d v_lin[st(r), i, h*dk+d] * msg[r,h,d,e]
 * A = rel_att (transpose_att = 0: the fused score <k . att, q>) or its transpose over (d, e) (1: <q . att, k>), st = src_type [R] int64
 * (device): the node type of every relation's sources.  The factors are the reference's, composed per edge there
 * (HGT/models.py:159-262: K_linear / V_linear per node type, relation_att, relation_pri / sqrt_dk, relation_msg).
 * k_lin, v_lin [T, K_in, H*dk]; rel_att, rel_msg [R,H,dk,dk]; rel_pri [R,H]; w_kv [R, K_in, 2*H*dk].  The backward overwrites all five
 * gradients (same shapes as the parameters). */
int het_hgt_fold_source_weights(const float* k_lin, const float* v_lin, const float* rel_att, const float* rel_msg,
                                const float* rel_pri, const int64_t* src_type, int64_t num_types, int64_t num_rels, int64_t H,
                                int64_t dk, int64_t K_in, int transpose_att, float* w_kv, het_stream stream);
int het_hgt_fold_source_weights_backward(const float* grad_w_kv, const float* k_lin, const float* v_lin, const float* rel_att,
                                         const float* rel_msg, const float* rel_pri, const int64_t* src_type, int64_t num_types,
                                         int64_t num_rels, int64_t H, int64_t dk, int64_t K_in, int transpose_att, float* grad_k_lin,
                                         float* grad_v_lin, float* grad_att, float* grad_msg, float* grad_pri, het_stream stream);

/* ------------------------------------------------------------------------
 * RGAT on the distinct (relation, node) rows without a per-edge float tensor (layer-level fusion; no reference op of
 * its own).  Replaces the pair relational_fused_gat_separate_coo / backward_... with CompactAsOfNodeKind 4
 * (OpExport/RGATOps.inc.h:170-245, 465-551; kernels RGAT/RGATKernelsSeparateCOO.cu.h:17-204,
 * RGATBackwardKernelsSeparateCOO.cu.h:9-117) inside the one-node RGAT layer: both passes form
 * exp(leaky_relu(el_c[srow] + er_c[drow])) from the compact tables instead of writing / re-reading exp [E,H].
 *   feat_c [S_row,H,D], el_c [S_row,H]: per distinct (relation, source) row;  er_c [S_col,H]: per (relation, destination)
 *   by_dst:  het_grouping_create(NULL, 0, col, E, N, payload0 = feat row of every position, payload1 = its er row)
 *   by_srow: het_grouping_create(NULL, 0, feat row of every position, E, S_row, payload0 = col, payload1 = er row)
 *   by_drow: het_grouping_create(NULL, 0, er row of every position, E, S_col, payload0 = rank of the position in by_srow
 *            (het_grouping_rank_of_position), NULL)
 * Softmax without overflow: the reference exponentiates the raw pre-activation (gatLeakyReluExp, GAT/FusedGAT.cu.h:23-26; the
 *   reference-named a4 / a5 keep that because exp and sum are API tensors there).  These two entry points subtract a running
 *   maximum per (destination, head): `sum` receives lse[v,h] = log(SUM_e exp(leaky_relu(el + er))) instead of the sum itself and
 *   the backward forms the attention weight as exp(leaky_relu(el + er) - lse[v,h]) -- the reference's value wherever its formula
 *   is finite, finite for any pre-activation.  The stored lse of a destination with in-edges is never exactly 0 (an exact 0 is
 *   stored as FLT_MIN), so `sum[v,h] == 0` -- the forward's zero fill -- marks a node without in-edges: the backward skips the
 *   `ret` rows of those nodes, so `sum` has to be the forward's output.  workspace (forward): het_rgat_aggregate_compact_workspace(by_dst, H, D) bytes,
 *   16-byte aligned (0 unless a destination has more than 256 in-edges: its work items park their partial sums there and a
 *   finishing pass brings them to one maximum -- no float atomics).
 * forward:  sum [N,H] (= lse), ret [N,H,D] are overwritten (a4's ret; exp is not produced).  h_inout [h_rows, H*D] (optional):
 *   the layer output so far (self-loop + bias, het_rows_linear_bias); ret's row is added to it in place for every
 *   destination < h_rows, and ret is then defined only for destinations WITH in-edges (no 0.5 GB zero fill).
 * backward: grad_feat_c, grad_el_c, grad_er_c are overwritten (a5's outputs on the compact rows).  fold_attn_l [R,H,D]
 *   (optional, with row_rel_ptrs [R+1] = relation pointers of the feat rows): adds grad_el_c[u,h] * fold_attn_l[r(u),h,:]
 *   into grad_feat_c -- the gradient through el_c = <feat_c, attn_l[r]>.  grad_bias [H*D] (optional): column sums of
 *   gradout's first bias_rows rows (the layer's bias gradient) from the pass that reads gradout anyway.
 *   workspace: het_rgat_backward_compact_workspace(N, E, H, D, grad_bias != NULL) bytes, 16-byte aligned. */
int het_rgat_aggregate_compact(const het_grouping* by_dst, const float* feat_c, const float* el_c, const float* er_c,
                               float* sum, float* ret, int64_t num_nodes, int64_t H, int64_t D, double slope,
                               float* h_inout, int64_t h_rows, void* workspace, int64_t workspace_bytes, het_stream stream);
int64_t het_rgat_aggregate_compact_workspace(const het_grouping* by_dst, int64_t H, int64_t D);
int64_t het_rgat_backward_compact_workspace(int64_t num_nodes, int64_t num_edges, int64_t H, int64_t D, int with_bias);
int het_rgat_backward_compact(const het_grouping* by_srow, const het_grouping* by_drow, const float* feat_c,
                              const float* el_c, const float* er_c, const float* sum, const float* ret,
                              const float* gradout, float* grad_feat_c, float* grad_el_c, float* grad_er_c,
                              const float* fold_attn_l, const int64_t* row_rel_ptrs, int64_t num_rels,
                              float* grad_bias, int64_t bias_rows, int64_t num_nodes, int64_t num_src_rows,
                              int64_t num_dst_rows, int64_t H, int64_t D, double slope, void* workspace,
                              int64_t workspace_bytes, het_stream stream);

/* The same pair with grad_er taken from per-RUN sums instead of a per-edge term (a run = the edges of one (relation,
 * destination) pair = one er row).  The reference's backward adds grad_er edge by edge with float atomics
 * (RGATBackwardKernelsSeparateCOO.cu.h:60-117); het_rgat_backward_compact writes a per-edge term [E,H] in (relation, source)
 * order and sums it in (relation, destination) order.  gradout[v] is common to a run, so the forward -- which visits the feat
 * rows of the run anyway -- can leave
 *   q_rows[w,h,:] = SUM_e w_e dl_e feat_c[srow_e,h,:],  q_sum[w,h] = SUM_e w_e dl_e,   w_e = exp(leaky(el + er) - q_ref[w,h]),
 *   dl_e = 1 or slope (the leaky-ReLU branch of edge e)
 * per er row w, and grad_er_c[w,h] = exp(q_ref[w,h] - lse[v,h]) (<gradout[v,h,:], q_rows[w,h,:]> - <gradout, ret>[v,h] q_sum[w,h]).
 *   by_dst_rel: het_grouping_create(NULL, 0, col * num_rels + relation of the position, E, N * num_rels, NULL, NULL) -- the same
 *     sorted order as by_dst when the positions are relation-major (a separate-COO list); its work items never cross a run.
 *   q_rows [S_col,H,D], q_sum / q_ref [S_col,H]: written by the forward, read by the backward.  drow_nodes [S_col] int64:
 *     destination node of every er row.  Shapes: rows of 32 / 64 / 128 floats with heads of >= 16 (else HET_ERR_UNSUPPORTED).
 *   attn_l [R,H,D] + feat_rel_ptrs_host (HOST array [R+1]: first feat row of every relation; feat rows are relation-major) --
 *     optional, both or neither: when el_c IS <feat_c[row,h,:], attn_l[relation of the row,h,:]> (the layer's case) the pass forms it
 *     from the row it gathers anyway instead of gathering el_c per edge (heads of 16 floats, up to 8 relations; el_c is still read
 *     by the other shapes and by the backward).
 *   workspaces: het_rgat_aggregate_compact_runs_workspace(by_dst, by_dst_rel, num_rels, H, D, stream) -- one record per work item of
 *     a destination with more than 128 in-edges (HET_RGAT_HUB_MIN); the first call lists those items on `stream` (kept with by_dst_rel and
 *     rebuilt if it is later used with another by_dst object); -1 on error;  het_rgat_backward_compact_runs_workspace (below) */
int64_t het_rgat_aggregate_compact_runs_workspace(const het_grouping* by_dst, const het_grouping* by_dst_rel, int64_t num_rels,
                                                  int64_t H, int64_t D, het_stream stream);
int het_rgat_aggregate_compact_runs(const het_grouping* by_dst, const het_grouping* by_dst_rel, int64_t num_rels,
                                    const float* feat_c, const float* el_c, const float* er_c, float* sum, float* ret,
                                    int64_t num_nodes, int64_t H, int64_t D, double slope, float* h_inout, int64_t h_rows,
                                    float* q_rows, float* q_sum, float* q_ref, int64_t num_dst_rows, const float* attn_l,
                                    const int64_t* feat_rel_ptrs_host, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_rgat_backward_compact_runs(const het_grouping* by_srow, const float* q_rows, const float* q_sum, const float* q_ref,
                                   const int64_t* drow_nodes, const float* feat_c, const float* el_c, const float* er_c,
                                   const float* sum, const float* ret, const float* gradout, float* grad_feat_c,
                                   float* grad_el_c, float* grad_er_c, const float* fold_attn_l, const int64_t* row_rel_ptrs,
                                   int64_t num_rels, float* grad_bias, int64_t bias_rows, int64_t num_nodes,
                                   int64_t num_src_rows, int64_t num_dst_rows, int64_t H, int64_t D, double slope,
                                   float* grad_attn_l, void* workspace, int64_t workspace_bytes, het_stream stream);
/* grad_attn_l [R,H,D] (optional; needs fold_attn_l, <= 8 relations): the weight gradient of el_c = <feat_c, attn_l[r]>,
 *   SUM_u grad_el_c[u,h] feat_c[u,h,:] per relation, overwritten -- formed from the rows the source-row kernels hold where a
 *   segment ends (per-workgroup partial rows + a finishing pass) instead of a row-dot pass that reads feat_c again.
 * workspace: het_rgat_backward_compact_runs_workspace(by_srow, N, num_dst_rows, H, D, grad_bias != NULL, grad_attn_l != NULL, stream)
 *   bytes (the first call with the attention gradient builds by_srow's packs on `stream`); -1 on error.  It holds, beside the
 *   per-destination {lse, <gradout, ret>} pairs, one 16-byte record {er, lse, <gradout, ret>, 0} per (er row, head): the source-row
 *   kernels fetch everything they need from the destination side of an edge with one load instead of two (round 4). */
int64_t het_rgat_backward_compact_runs_workspace(const het_grouping* by_srow, int64_t num_nodes, int64_t num_dst_rows, int64_t H,
                                                 int64_t D, int with_bias, int with_attn_grad, het_stream stream);
/* het_rgat_backward_compact_runs in two halves, for a caller whose next launch needs grad_feat_c / grad_er_c but not grad_attn_l (the
 * RGAT layer: its node-major input gradient starts where the edge pass ends, the finishing pass runs beside it on another stream):
 *   het_rgat_backward_compact_runs_edges: the same arguments, the same launches and the same values, except that the partial rows of
 *     grad_attn_l are left in the workspace.  grad_attn_l then holds the zero fill plus the few boundary pieces added atomically.
 *   het_rgat_attn_grad_finish: grad_attn_l[r, :] += the partial rows tagged r.  by_srow, num_nodes, num_dst_rows, num_rels, H, D and
 *     with_bias (= grad_bias != NULL) as the edge pass was given them -- they say where the partial rows lie in `workspace`, which
 *     nobody may have written since.  `stream` must be ordered after the edge pass (its own stream, or one that waits for it).
 *     Nothing to do (HET_OK) when the grouping has no position.
 * het_rgat_backward_compact_runs is the one followed by the other on `stream`: bit for bit what the two calls leave. */
int het_rgat_backward_compact_runs_edges(const het_grouping* by_srow, const float* q_rows, const float* q_sum, const float* q_ref,
                                         const int64_t* drow_nodes, const float* feat_c, const float* el_c, const float* er_c,
                                         const float* sum, const float* ret, const float* gradout, float* grad_feat_c,
                                         float* grad_el_c, float* grad_er_c, const float* fold_attn_l, const int64_t* row_rel_ptrs,
                                         int64_t num_rels, float* grad_bias, int64_t bias_rows, int64_t num_nodes,
                                         int64_t num_src_rows, int64_t num_dst_rows, int64_t H, int64_t D, double slope,
                                         float* grad_attn_l, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_rgat_attn_grad_finish(const het_grouping* by_srow, int64_t num_nodes, int64_t num_dst_rows, int64_t num_rels, int64_t H,
                              int64_t D, int with_bias, float* grad_attn_l, void* workspace, int64_t workspace_bytes,
                              het_stream stream);

/* The forward of that pair when no backward will follow (evaluation, torch.no_grad()): the same groupings -- by_dst and by_dst_rel
 * as for het_rgat_aggregate_compact_runs, so a training step and an evaluation pass over one graph share them --, the same feat_c /
 * el_c / er_c / slope / attn_l / feat_rel_ptrs_host, and ONE output:
 *   h_inout [h_rows, H*D] (required, 16-byte aligned): h_inout[v] += SUM_e softmax_v(leaky(el + er))_e feat_c[srow_e] in place for
 *     every destination v < h_rows that has in-edges; the other rows are not touched (a caller without a self-loop term passes
 *     zeros).  Neither lse, ret nor the run sums are formed or stored -- on an ogbn-mag-sized graph that is 0.8 GB the training
 *     forward writes for its backward.  The value of every row is bit for bit what het_rgat_aggregate_compact_runs leaves in its
 *     h_inout for the same arguments (same operations, same order, same roundings).
 *   Shapes as there (else HET_ERR_UNSUPPORTED); null groupings, a null or misaligned h_inout and groupings of the wrong shape are
 *   HET_ERR_INVALID_ARG; nothing is enqueued before these checks pass.  No edges: HET_OK, h_inout untouched.
 *   workspace: het_rgat_aggregate_compact_forward_workspace(by_dst, by_dst_rel, num_rels, H, D, stream) bytes, 16-byte aligned -- one
 *     record {O[H*D], max[H], sum[H]} per work item of a hub destination (num_hub_items * (H*D + 2*H) floats); lists those items on
 *     `stream` on first use, as its twin does; -1 on error. */
int64_t het_rgat_aggregate_compact_forward_workspace(const het_grouping* by_dst, const het_grouping* by_dst_rel, int64_t num_rels,
                                                     int64_t H, int64_t D, het_stream stream);
int het_rgat_aggregate_compact_forward(const het_grouping* by_dst, const het_grouping* by_dst_rel, int64_t num_rels,
                                       const float* feat_c, const float* el_c, const float* er_c, int64_t H, int64_t D, double slope,
                                       float* h_inout, int64_t h_rows, const float* attn_l, const int64_t* feat_rel_ptrs_host,
                                       void* workspace, int64_t workspace_bytes, het_stream stream);

/* ... with bf16 activation rows (the RGAT layer's evaluation path on a torch.bfloat16 input): feat_c [S_row,H,D] and h_inout
 * [h_rows, H*D] are het_bf16, both 16-byte aligned (else HET_ERR_INVALID_ARG, nothing enqueued); el_c, er_c, attn_l, the hub records
 * of the workspace, every maximum, exponential and sum are fp32.  Arguments, checks, shapes and workspace
 * (het_rgat_aggregate_compact_forward_workspace) are het_rgat_aggregate_compact_forward's.  Rows are widened on load (exact); a
 * lane holds the same 4 elements of a row as in the fp32 kernels, so the sums are formed in the same order; the one rounding (to
 * nearest even) is at the store: h_inout[v] = round(widen(h_inout[v]) + SUM_e softmax_v(..)_e widen(feat_c[srow_e])) for every
 * destination v < h_rows with in-edges, the other rows are not touched.  No float atomics.
 *   el_c [S_row,H] must hold <widen(feat_c[u,h,:]), attn_l[r(u),h,:]> -- the dots of the ROUNDED rows (het_rgat_el_rows_bf16) --, which
 *   is the function the walk itself computes where it forms el from the gathered row (attn_l and feat_rel_ptrs_host given, D == 16,
 *   num_rels <= 8); in that case el_c is never read and may be NULL.
 * het_rgat_el_rows_bf16: that el_c from feat_c [num_rows,H,D] het_bf16 (rows relation-major, rel_ptrs [num_rels+1] on the device) and
 *   attn_l [num_rels,H,D]; fp32 products and sums, el_c [num_rows,H] fp32.  Same shapes. */
int het_rgat_aggregate_compact_forward_bf16(const het_grouping* by_dst, const het_grouping* by_dst_rel, int64_t num_rels,
                                            const het_bf16* feat_c, const float* el_c, const float* er_c, int64_t H, int64_t D,
                                            double slope, het_bf16* h_inout, int64_t h_rows, const float* attn_l,
                                            const int64_t* feat_rel_ptrs_host, void* workspace, int64_t workspace_bytes,
                                            het_stream stream);
int het_rgat_el_rows_bf16(const int64_t* rel_ptrs, int64_t num_rels, const het_bf16* feat_c, const float* attn_l, float* el_c,
                          int64_t num_rows, int64_t H, int64_t D, het_stream stream);

/* The TRAINING pair with bf16 activation rows (the RGAT layer built with bf16_training=True): het_rgat_aggregate_compact_runs and
 * het_rgat_backward_compact_runs with feat_c [S_row,H,D], h_inout [h_rows, H*D] and gradout [rows,H,D] as het_bf16; el_c, er_c, sum
 * (the log-sum-exp), ret, the run sums q_rows / q_sum / q_ref, the hub records of the workspace, rec4 and every gradient are fp32.
 * Arguments, shapes, groupings and workspaces (het_rgat_aggregate_compact_runs_workspace, het_rgat_backward_compact_runs_workspace)
 * are the fp32 entries'.  Rows are widened on load (exact); a lane holds the same 4 elements of a row as in the fp32 kernels (8 bytes
 * instead of 16), so every sum is formed in the fp32 order.
 *   forward: ret[v] is the fp32 acc * rcp(sum), not rounded; h_inout[v] = round(widen(h_inout[v]) + ret[v]) (to nearest even) for
 *     every destination v < h_rows with in-edges -- bit for bit what het_rgat_aggregate_compact_forward_bf16 stores.  el_c is required
 *     (the backward reads it) and must hold the dots of the ROUNDED rows (het_rgat_el_rows_bf16).
 *   backward: the run-sum form on the cooperative shapes only; grad_bias, when asked for, is the column sums of the bf16 gradout rows
 *     [0, bias_rows).  The gradient passes straight through the rounding of feat_c: grad_feat_c is that of the widened rows.
 *   The bf16 rows must be 8-byte aligned, every fp32 table and the workspace 16-byte aligned, h_rows <= num_nodes: else
 *     HET_ERR_INVALID_ARG; other shapes HET_ERR_UNSUPPORTED; nothing is enqueued before these checks pass. */
int het_rgat_aggregate_compact_runs_bf16(const het_grouping* by_dst, const het_grouping* by_dst_rel, int64_t num_rels,
                                         const het_bf16* feat_c, const float* el_c, const float* er_c, float* sum, float* ret,
                                         int64_t num_nodes, int64_t H, int64_t D, double slope, het_bf16* h_inout, int64_t h_rows,
                                         float* q_rows, float* q_sum, float* q_ref, int64_t num_dst_rows, const float* attn_l,
                                         const int64_t* feat_rel_ptrs_host, void* workspace, int64_t workspace_bytes,
                                         het_stream stream);
int het_rgat_backward_compact_runs_bf16(const het_grouping* by_srow, const float* q_rows, const float* q_sum, const float* q_ref,
                                        const int64_t* drow_nodes, const het_bf16* feat_c, const float* el_c, const float* er_c,
                                        const float* sum, const float* ret, const het_bf16* gradout, float* grad_feat_c,
                                        float* grad_el_c, float* grad_er_c, const float* fold_attn_l, const int64_t* row_rel_ptrs,
                                        int64_t num_rels, float* grad_bias, int64_t bias_rows, int64_t num_nodes,
                                        int64_t num_src_rows, int64_t num_dst_rows, int64_t H, int64_t D, double slope,
                                        float* grad_attn_l, void* workspace, int64_t workspace_bytes, het_stream stream);
/* ... its first half (het_rgat_backward_compact_runs_edges above; the second half, het_rgat_attn_grad_finish, is fp32 either way) */
int het_rgat_backward_compact_runs_edges_bf16(const het_grouping* by_srow, const float* q_rows, const float* q_sum, const float* q_ref,
                                              const int64_t* drow_nodes, const het_bf16* feat_c, const float* el_c, const float* er_c,
                                              const float* sum, const float* ret, const het_bf16* gradout, float* grad_feat_c,
                                              float* grad_el_c, float* grad_er_c, const float* fold_attn_l,
                                              const int64_t* row_rel_ptrs, int64_t num_rels, float* grad_bias, int64_t bias_rows,
                                              int64_t num_nodes, int64_t num_src_rows, int64_t num_dst_rows, int64_t H, int64_t D,
                                              double slope, float* grad_attn_l, void* workspace, int64_t workspace_bytes,
                                              het_stream stream);

/* The attention weights the aggregations above form and discard, as an output (DGL's get_attention, PyG's
 * return_attention_weights): a pass of its own over the ids and the two small tables -- it never reads a feat_c row, and it runs
 * after either evaluation entry (el_c / er_c are fp32 in the bf16 layer too; everything here is fp32).
 *   attn [num_edges, H] (required): attn[row(p), h] = exp(leaky(el_c[srow[p], h] + er_c[drow[p], h]) - lse[col[p], h]) for every edge
 *     position p, row(p) = eids[p], or p when eids is NULL; eids must be a permutation of [0, num_edges).  Every row is written.
 *   lse_out [num_nodes, H] (optional): lse[v, h] = log SUM_{p: col[p] == v} exp(leaky(..)), formed relative to a running maximum (any
 *     score is safe); -inf for a destination without in-edges.  Without it the rows live in the workspace.
 *   by_dst: the grouping of the positions by destination with payload0 = srow and payload1 = drow (the one
 *     het_rgat_aggregate_compact_forward takes); col / srow / drow / eids [num_edges] int64 on the device are the lists it was built
 *     from.  Destinations of more than 256 in-edges are split over work items whose {max[H], sum[H]} records meet in a finishing
 *     launch, in a fixed order: no float atomics, the same bits from run to run.
 *   H in {1, 2, 4, 8}, num_nodes and num_edges below 2^31: HET_ERR_UNSUPPORTED otherwise.  A null grouping, a null el_c / er_c / col /
 *     srow / drow / attn, a pointer off its alignment (16 bytes for the float tensors and the workspace, 8 for the id lists), a
 *     grouping of another shape and a workspace that is too small are HET_ERR_INVALID_ARG; nothing is enqueued before these checks
 *     pass.  num_edges == 0: HET_OK, nothing is touched; by_dst is still required then (and must group no positions), no other
 *     pointer is looked at.
 *   workspace: het_rgat_attention_compact_workspace(by_dst, H, num_nodes, lse_out != NULL) bytes, 16-byte aligned -- the lse rows
 *     when lse_out is NULL, and one {max[H], sum[H]} record per work item when the grouping has split destinations; -1 on error. */
int64_t het_rgat_attention_compact_workspace(const het_grouping* by_dst, int64_t H, int64_t num_nodes, int with_lse_out);
int het_rgat_attention_compact(const het_grouping* by_dst, const float* el_c, const float* er_c, int64_t H, double slope,
                               const int64_t* col, const int64_t* srow, const int64_t* drow, const int64_t* eids, int64_t num_edges,
                               int64_t num_nodes, float* lse_out, float* attn, void* workspace, int64_t workspace_bytes,
                               het_stream stream);

/* The two halves of a2 (backward_rgnn_relational_matmul, one input head, matrix-core shapes) as separate calls, so that a
 * caller can order them around a collective (het_amd/dist.py).  Rows i in [0, num_rows) of relation-bucketed lists:
 *   dx: grad_x[gather_idx[i], :] (+)= gradout[g_rows[i], :] . Wt[r(i)]      atomic 0: "=";  1: "+=" with float atomics (rows
 *       may repeat);  2: "+=" for lists whose gather_idx are distinct inside every relation (a unique (relation, node)
 *       list): relation by relation with plain read-modify-write (up to 8 relations, atomics beyond)
 *   dw: grad_w[r(i)]             (+)= x[gather_idx[i], :]^T (x) gradout[g_rows[i], :]
 * gather_idx / g_rows NULL = row i.  weights_t [R,H,D,K], grad_w [R,H,K,D]. */
int het_rows_matmul_backward_dx(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx, const int64_t* g_rows,
                                int64_t num_rows, const float* weights_t, const float* gradout, float* grad_x, int64_t H,
                                int64_t K, int64_t D, int atomic, het_stream stream);
int het_rows_matmul_backward_dw(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx, const int64_t* g_rows,
                                int64_t num_rows, const float* x, const float* gradout, float* grad_w, int64_t H, int64_t K,
                                int64_t D, int accumulate, het_stream stream);
/* The same with the column sums of the gradout rows of the launch from the same pass: colsum[H*D] = SUM_i gradout[g_rows[i], :]
 * (always "="; NULL: none).  For a list that names every output row once (the self-loop product of the RGAT layer,
 * RGAT/models.py:378-381) that is the bias gradient, which otherwise costs its own pass over gradout. */
int het_rows_matmul_backward_dw_colsum(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx,
                                       const int64_t* g_rows, int64_t num_rows, const float* x, const float* gradout,
                                       float* grad_w, float* colsum, int64_t H, int64_t K, int64_t D, int accumulate,
                                       het_stream stream);

/* Row products with bf16 activation rows (the HGT layer with bf16 activations; fp32 weights, fp32 accumulation on the matrix cores):
 *   het_rows_matmul_bf16:             out[scatter_idx[i], :] = x[gather_idx[i], :] . weights[r(i)]     x [*,K], out [*,X] het_bf16 (x
 *       widened on load -- exact --, out rounded once at the store), weights [R,K,X] fp32; plain stores (the listed output rows
 *       are distinct); gather_idx / scatter_idx NULL = row i.  K in {32, 64}, X in {32, 64, 128}; else HET_ERR_UNSUPPORTED.
 *   het_rows_matmul_heads_bf16:       out[i, (h,d)] = x[gather_idx[i], :] . weights[r(i), h, :, d]     the same product with the weight
 *       in the RGAT layer's head-concatenated layout [R,H,K,D] and out [num_rows, H*D] in list order (feat_c on the distinct
 *       (relation, node) rows).  K and H*D in {32, 64, 128} (an input width zero-padded to 128 included).
 *   het_rows_matmul_backward_dw_bf16: grad_w[r(i)] (+)= x[gather_idx[i], :]^T (x) gradout[g_rows[i], :]   x [*,K] het_bf16; gradout
 *       [*,X] fp32, or het_bf16 for het_rows_matmul_backward_dw_bf16_bf16; grad_w [R,K,X] fp32.  K in {32, 64}, X in {32, 64, 128}.
 *   het_rows_dot1h_bf16:              out[scatter_idx[i], h] = <x[gather_idx[i], :], weights[r(i), h, :]>     x [*,K] het_bf16 (widened on
 *       load), weights [R,H,K] and out [*,H] fp32, fp32 products and sums: one input row against the H vectors of its relation (er_c
 *       of the RGAT layer from the folded weight W . attn_r, no fp32 copy of x).  H in {1, 2, 4, 8}, K a power of two in [4 H, 256]. */
int het_rows_matmul_bf16(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx, const int64_t* scatter_idx,
                         int64_t num_rows, const float* weights, const het_bf16* x, het_bf16* out, int64_t K, int64_t X,
                         het_stream stream);
int het_rows_matmul_backward_dw_bf16(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx, const int64_t* g_rows,
                                     int64_t num_rows, const het_bf16* x, const float* gradout, float* grad_w, int64_t K, int64_t X,
                                     int accumulate, het_stream stream);
int het_rows_matmul_backward_dw_bf16_bf16(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx, const int64_t* g_rows,
                                          int64_t num_rows, const het_bf16* x, const het_bf16* gradout, float* grad_w, int64_t K,
                                          int64_t X, int accumulate, het_stream stream);
int het_rows_matmul_heads_bf16(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx, int64_t num_rows,
                               const float* weights, const het_bf16* x, het_bf16* out, int64_t H, int64_t K, int64_t D,
                               het_stream stream);
int het_rows_dot1h_bf16(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx, const int64_t* scatter_idx,
                        int64_t num_rows, const float* weights, const het_bf16* x, float* out, int64_t H, int64_t K,
                        het_stream stream);
/* ... and its weight gradient: grad_w[r, h, :] (+)= SUM_i gradout[scatter_idx[i], h] * x[gather_idx[i], :]     x [*,K] het_bf16 (8-byte
 * aligned), gradout [*,H] and grad_w [R,H,K] fp32 (16-byte aligned).  accumulate 0: grad_w is cleared first; workgroups add their
 * partial rows with float atomics.  Same shapes. */
int het_rows_dot1h_backward_dw_bf16(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* gather_idx, const int64_t* scatter_idx,
                                    int64_t num_rows, const het_bf16* x, const float* gradout, float* grad_w, int64_t H, int64_t K,
                                    int accumulate, het_stream stream);

/* ------------------------------------------------------------------------
 * Node-major input gradient of the one-node RGAT layer (layer-level fusion; no reference op of its own).  It replaces,
 * inside het_amd/backend/rgat_fused_layer.py, the per-relation input-gradient passes of a2 (backward_rgnn_relational_matmul
 * with CompactAsOfNodeKind 1, OpExport/RGNNOps.inc.h:946-1010 -> kernels RGNN/my_shmem_sgemm_func.cu.h:711-776), the self-loop's
 * a3 backward (RGNNOps.inc.h:660-753) and the D_out = 1 product of the attention-vector side: ONE pass over the nodes forms
 *   grad_x[n,:]  = grad_h[n,:] . loop_wt  +  SUM_r g_rows[row_map[r,n],:] . weights_t[r]  +  SUM_r,h g_er[dst_map[r,n],h] * wa_t[r,h,:]
 * for the nodes n in [n_begin, n_end) and stores the row once; terms whose map entry is -1 (and the grad_h term for
 * n >= n_loop) are absent.
 *   row_map / dst_map [R, num_nodes] int32: row of (relation, node) in the unique (relation, source) / (relation,
 *   destination) list, -1 if the node has none (het_node_row_map);  grad_h [n_loop, H*D];  g_rows [S_row, H*D];
 *   g_er [S_col, H] (NULL: no such term);  loop_wt [H*D, K] (= loop_weight^T);  weights_t [R,H,D,K];  wa_t [R,H,K].
 *   node_order [num_nodes] int32 (optional): positions [n_begin, n_end) of this list are the nodes of the call (NULL: node p at
 *   position p).  The kernel multiplies 32-node tiles per relation that has a row in the tile; a list sorted by WHICH relations a
 *   node has rows in makes the tiles homogeneous (no zero rows: 26 % fewer matrix-core instructions on ogbn-mag).
 *   Shapes: K and H*D in {32, 64}, H in {1,2,4,8}, R*H <= 32, all 1 + R weights resident in LDS (het_rgat_node_gemm_ok);
 *   HET_ERR_INVALID_ARG otherwise -- callers fall back to the per-relation entry points. */
int het_rgat_node_gemm_ok(int64_t num_rels, int64_t H, int64_t K, int64_t D);
int het_node_row_map(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* nodes, int64_t num_rows, int64_t num_nodes,
                     int32_t* map, het_stream stream);
int het_rgat_node_backward_dx(int64_t n_begin, int64_t n_end, int64_t n_loop, int64_t num_nodes, int64_t num_rels,
                              const float* grad_h, const float* loop_wt, const float* g_rows, const float* weights_t,
                              const int32_t* row_map, const float* g_er, const float* wa_t, const int32_t* dst_map,
                              float* grad_x, int64_t H, int64_t K, int64_t D, const int32_t* node_order, het_stream stream);
/* ... with bf16 activation rows: grad_h [n_loop, H*D] and grad_x [num_nodes, K] het_bf16 (8-byte aligned; grad_h widened on load,
 * grad_x rounded once, to nearest even, after every term of the node is summed); g_rows, g_er and the weights fp32 (16-byte aligned). */
int het_rgat_node_backward_dx_bf16(int64_t n_begin, int64_t n_end, int64_t n_loop, int64_t num_nodes, int64_t num_rels,
                                   const het_bf16* grad_h, const float* loop_wt, const float* g_rows, const float* weights_t,
                                   const int32_t* row_map, const float* g_er, const float* wa_t, const int32_t* dst_map,
                                   het_bf16* grad_x, int64_t H, int64_t K, int64_t D, const int32_t* node_order, het_stream stream);
/* The parameter forms of one step of that layer, a launch each (they depend on the parameters alone: the layer makes them once per
 * step, in the forward, and keeps them for the backward).
 * het_rgat_transpose_weights: weights_t [R,H,D,K] = weights [R,H,K,D] with the last two axes swapped, and -- loop_w given --
 *   loop_wt [X,K] = loop_w [K,X] transposed, both in ONE launch.  Exact copies (bit for bit a transposed contiguous copy); no
 *   alignment is asked of any pointer; the copies cannot be made in place.  K, D, X < 32768.
 * het_rgat_unfold_weight_gradient: the gradient through the folded weight wa[r,h,k] = SUM_d weights[r,h,k,d] attn_r[r,h,d], from
 *   grad_wa [R,H,K]:  grad_weights[r,h,k,d] += grad_wa[r,h,k] attn_r[r,h,d] in place, and grad_attn_r[r,h,d] = SUM_k
 *   weights[r,h,k,d] grad_wa[r,h,k], overwritten.  One workgroup per (r, h); fp32 sums over k in a fixed order, no float atomics: the
 *   same bits every call. */
int het_rgat_transpose_weights(const float* weights, int64_t num_rels, int64_t H, int64_t K, int64_t D, float* weights_t,
                               const float* loop_w, int64_t X, float* loop_wt, het_stream stream);
int het_rgat_unfold_weight_gradient(const float* grad_wa, const float* weights, const float* attn_r, int64_t num_rels, int64_t H,
                                    int64_t K, int64_t D, float* grad_weights, float* grad_attn_r, het_stream stream);

/* Layer-level extension (no reference op of its own): the node-major sum of row x weight products
 *     out[n, :] = SUM_s rows_s[map_s[n], :] . weights_t[s]          n = node_order[p] (or p) for p in [n_begin, n_end)
 * -- the input gradient of a layer input that feeds several projections, formed in ONE pass over the nodes instead of one
 * read-modify-write (the reference: float-atomic) pass per projection: replaces the a2 / a3 input-gradient launches behind the
 * HGT layer (backward_rgnn_relational_matmul / ..._no_scatter_gather_list, OpExport/RGNNOps.inc.h:946-1010, 660-753, as
 * HGT/models.py:159-262 composes them).  Source s: rows[s] = its first row (a column offset into a wider row is part of the
 * pointer: the k' and the m half of HGT's [S_row, 2X] gradient are two sources), row_strides[s] floats between rows,
 * maps[s] [num_nodes] int32 = row of node n or -1 (het_node_row_map gives [R, N] of them), or NULL: row = n for
 * n < ident_rows[s]; weights_t[s] [KS, XO] row-major (the projection's weight transposed).  Every node of the range is
 * written (zeros where it has no row).  KS, XO in {32, 64}; all weights of a call stay in LDS: at most 9 sources and
 * het_node_rows_matmul_sum_ok(num_sources, KS, XO).  node_order as in het_rgat_node_backward_dx. */
int het_node_rows_matmul_sum_ok(int64_t num_sources, int64_t KS, int64_t XO);
int het_node_rows_matmul_sum(int64_t n_begin, int64_t n_end, int64_t num_nodes, int64_t num_sources,
                             const float* const* rows, const int64_t* row_strides, const int32_t* const* maps,
                             const int64_t* ident_rows, const float* const* weights_t, float* out, int64_t KS, int64_t XO,
                             const int32_t* node_order, het_stream stream);

/* the same with a bias row: out[n, :] = bias[:] + SUM_s ...   (bias [XO] or NULL; a node without any row gets the bias) */
int het_node_rows_matmul_sum_bias(int64_t n_begin, int64_t n_end, int64_t num_nodes, int64_t num_sources,
                                  const float* const* rows, const int64_t* row_strides, const int32_t* const* maps,
                                  const int64_t* ident_rows, const float* const* weights_t, const float* bias, float* out,
                                  int64_t KS, int64_t XO, const int32_t* node_order, het_stream stream);

/* het_node_rows_matmul_sum with het_bf16 output rows: the source rows, the weights and the sums are fp32, every output row is
 * rounded once after all of a node's terms are added (the input gradient of the HGT layer with bf16 activations). */
int het_node_rows_matmul_sum_bf16(int64_t n_begin, int64_t n_end, int64_t num_nodes, int64_t num_sources,
                                  const float* const* rows, const int64_t* row_strides, const int32_t* const* maps,
                                  const int64_t* ident_rows, const float* const* weights_t, het_bf16* out, int64_t KS, int64_t XO,
                                  const int32_t* node_order, het_stream stream);

/* ------------------------------------------------------------------------
 * The RGCN layer as two calls (layer-level fusion; no reference op of its own).  Inside het_amd/backend/rgcn_layers_and_funcs.py
 * it replaces the pair a7 / a8 (rgcn_layer1_separate_coo / backward_rgcn_layer1_separate_coo, OpExport/RGCNOps.inc.h:84-138,
 * 368-467) together with the layer's "node_repr + h_bias" (RGCN/RGCN.py:338-340) and the fills the
 * reference wrappers make around the ops (rgcn_layers_and_funcs.py:481-601).  Same values:
 *   forward   ssum[(r,v), :] = SUM over the in-edges e of v in relation r of norm[eid_e] * x[src_e, :]       (kept for the backward)
 *             ret[v, :]      = bias[:] + SUM_r ssum[(r,v), :] . W[r]          one pass over the nodes, every row stored once
 *   backward  gsum[(r,u), :] = SUM over the out-edges e of u in relation r of norm[eid_e] * gradout[dst_e, :]
 *             grad_x[u, :]   = SUM_r gsum[(r,u), :] . Wt[r]                   one pass over the nodes, every row stored once
 *             grad_w[r]      = SUM over the (r,v) rows of ssum[(r,v), :]^T (x) gradout[v, :];   grad_bias = column sums of gradout
 *             (grad_w and grad_bias on the library's side stream beside the gather pass; joined before the call returns)
 * by_rel_dst = het_grouping_create(rel_ptrs, R, col, E, N_dst, payload0 = row, payload1 = eids), by_rel_src = the same with row
 * and col exchanged (the groupings of a7 / a8).  dst_map / src_map [R, N] int32: segment of (relation, node) in that grouping =
 * its row in the sorted unique (relation, node) list, -1 = none (het_grouping_segment_map).  node_order: optional, as in
 * het_rgat_node_backward_dx.  norm [E] by edge id, or norm_sorted [E] in the order of the call's gather grouping (by_rel_dst forward,
 * by_rel_src backward: het_grouping_gather_payload1; ogbn-mag: the forward's gather pass 0.85 -> see DESIGN.md 4.5) -- one of the two
 * may be NULL.  ssum [by_rel_dst segments, K];  weights [R,K,D];  weights_t [R,D,K];  bias / grad_bias [D] or NULL.
 * Shapes: K, D in {32, 64}, all R weights resident in LDS (het_rgcn_layer_ok); HET_ERR_INVALID_ARG otherwise -- callers use a7 / a8.
 * workspace: het_rgcn_layer_backward_workspace(segments of by_rel_src, D) bytes, 16-byte aligned.  grad_x NULL: the layer input
 * needs no gradient (fixed features): only grad_w / grad_bias are formed -- no gather pass. */
int het_rgcn_layer_ok(int64_t num_rels, int64_t K, int64_t D);
int64_t het_rgcn_layer_backward_workspace(int64_t n_src_rows, int64_t D);
int het_rgcn_layer_forward(const het_grouping* by_rel_dst, int64_t num_rels, int64_t num_nodes, const float* x,
                           const float* weights, const float* norm, const float* norm_sorted, const float* bias,
                           const int32_t* dst_map, const int32_t* node_order, float* ssum, float* ret, int64_t K, int64_t D,
                           het_stream stream);
int het_rgcn_layer_backward(const het_grouping* by_rel_src, const het_grouping* by_rel_dst, int64_t num_rels,
                            int64_t num_src_nodes, int64_t num_dst_nodes, const float* ssum, const float* weights_t,
                            const float* norm, const float* norm_sorted, const float* gradout, const int32_t* src_map,
                            const int32_t* node_order, float* grad_x, float* grad_w, float* grad_bias, int64_t K, int64_t D, void* workspace,
                            int64_t workspace_bytes, het_stream stream);
/* The same layer with bf16 activations: x, ret, gradout and grad_x are het_bf16 rows; the weights, norm, bias, ssum, the workspace,
 * grad_w and grad_bias stay fp32, as do all sums.  bf16 values are widened on load (exact) and ret / grad_x are rounded once, to
 * nearest even, when stored (after the fp32 bias is added).  Arguments, shapes, workspace and validation as the fp32 pair. */
int het_rgcn_layer_forward_bf16(const het_grouping* by_rel_dst, int64_t num_rels, int64_t num_nodes, const het_bf16* x,
                                const float* weights, const float* norm, const float* norm_sorted, const float* bias,
                                const int32_t* dst_map, const int32_t* node_order, float* ssum, het_bf16* ret, int64_t K, int64_t D,
                                het_stream stream);
int het_rgcn_layer_backward_bf16(const het_grouping* by_rel_src, const het_grouping* by_rel_dst, int64_t num_rels,
                                 int64_t num_src_nodes, int64_t num_dst_nodes, const float* ssum, const float* weights_t,
                                 const float* norm, const float* norm_sorted, const het_bf16* gradout, const int32_t* src_map,
                                 const int32_t* node_order, het_bf16* grad_x, float* grad_w, float* grad_bias, int64_t K, int64_t D,
                                 void* workspace, int64_t workspace_bytes, het_stream stream);

/* ------------------------------------------------------------------------
 * The RGCN layer with block-diagonal relation weights (DGL's RelGraphConv(regularizer="bdd"); RGCN/RGCN.py names the regularizer,
 * the reference does not implement it).  B blocks, si = K / B, so = D / B, weights [R, B, si, so]:
 *   out[v, b*so + j] = bias[b*so + j] + SUM_r SUM_{e: rel r, dst v} norm[eid_e] * SUM_i x[src_e, b*si + i] * weights[r, b, i, j]
 * as the two-call layer above with its node passes and its weight gradient replaced:
 *   forward   ssum[(r,v), :]   = SUM over the in-edges e of v in relation r of norm[eid_e] * x[src_e, :]     (kept for the backward)
 *             ret[v, :]        = bias + SUM over the entries (r, row) of v of ssum[row, :] . blockdiag(weights[r])
 *   backward  gsum[(r,u), :]   = SUM over the out-edges e of u in relation r of norm[eid_e] * gradout[dst_e, :]
 *             grad_x[u, :]     = SUM over the entries (r, row) of u of gsum[row, :] . blockdiag(weights[r])^T
 *             grad_w[r, b]     = SUM over the rows (r,v) of ssum[row, block b]^T (x) gradout[v, block b];  grad_bias = column sums of gradout
 * Summation order: the entries of a node in ascending relation order, one fused multiply-add per term, the bias last; the rows of
 * a relation in chunks of het_rgcn_bdd_params()[0] rows (inside a chunk: 256 / D interleaved row groups, then the groups in order),
 * the chunk partials in chunk order.  No float atomics and no buffer the caller has to fill: a node without entries gets the bias
 * (or zeros), a relation without rows gets a zero gradient; the same inputs give the same bits (the gather-sum adds the parts of a
 * split segment atomically -- only segments of more than 256 edges are split).
 *
 * het_grouping_node_rows: the per-node list of a grouping by (relation, key) -- node_ptr [num_keys + 1], and per entry the segment
 * (ent_row [S]: the row of ssum / gsum) and its relation (ent_rel [S]); S = het_grouping_num_segments.  Built on the device from the
 * grouping's segment list by a stable sort by key, so a node's entries are in ascending relation order; nothing is read back.  It
 * replaces the [R, N] map of het_grouping_segment_map: ent_row[node_ptr[n] ..] are the non-negative values of map[:, n], in order.
 * The forward takes the list of by_rel_dst, the backward that of by_rel_src.
 *
 * Shapes (het_rgcn_bdd_layer_ok): fp32, K and D in {32, 64, 128}, si and so in {4, 8, 16, 32}, any R >= 1, fewer than 2^31 nodes;
 * HET_ERR_UNSUPPORTED otherwise.  Bad counts, null or misaligned pointers (16 bytes: x, weights, bias, ssum, ret, gradout, grad_x,
 * grad_w, workspace), a missing grouping or a short workspace: HET_ERR_INVALID_ARG.  Either answer names the entry and comes before
 * anything is enqueued.  weights_t [R, B, so, si]: every block transposed.  workspace: het_rgcn_bdd_layer_backward_workspace(segments
 * of by_rel_src, segments of by_rel_dst, R, K, D, B) bytes (-1: bad arguments).  grad_x NULL: no source-side gather and no node pass.
 * The blocks of all relations are held in LDS while R * K * D / B * 4 <= het_rgcn_bdd_params()[1] bytes and read through the caches
 * beyond.  het_rgcn_bdd_params(out[6]): chunk rows, LDS weight bytes, threads per workgroup, smallest and largest block side, column
 * sum workgroups. */
int het_grouping_node_rows(const het_grouping* g, int64_t num_keys, int32_t* node_ptr, int32_t* ent_row, int32_t* ent_rel,
                           het_stream stream);
int het_rgcn_bdd_layer_ok(int64_t num_rels, int64_t K, int64_t D, int64_t B);
int64_t het_rgcn_bdd_layer_backward_workspace(int64_t n_src_rows, int64_t n_dst_rows, int64_t num_rels, int64_t K, int64_t D, int64_t B);
int het_rgcn_bdd_layer_forward(const het_grouping* by_rel_dst, int64_t num_rels, int64_t num_nodes, const float* x,
                               const float* weights, const float* norm, const float* norm_sorted, const float* bias,
                               const int32_t* node_ptr, const int32_t* ent_row, const int32_t* ent_rel, float* ssum, float* ret,
                               int64_t K, int64_t D, int64_t B, het_stream stream);
int het_rgcn_bdd_layer_backward(const het_grouping* by_rel_src, const het_grouping* by_rel_dst, int64_t num_rels,
                                int64_t num_src_nodes, int64_t num_dst_nodes, const float* ssum, const float* weights_t,
                                const float* norm, const float* norm_sorted, const float* gradout, const int32_t* node_ptr,
                                const int32_t* ent_row, const int32_t* ent_rel, float* grad_x, float* grad_w, float* grad_bias,
                                int64_t K, int64_t D, int64_t B, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_rgcn_bdd_params(int64_t* out);

/* self-loop + bias of a layer as one pass (RGAT/models.py:378-381: h + th.matmul(inputs_dst, loop_weight) + h_bias):
 * out[i,:] = x[i,:] . w + bias for rows [offsets[0], offsets[1]) (offsets: device array), w [K,X], bias [X] or NULL.
 * Matrix-core shapes only (HET_ERR_UNSUPPORTED otherwise). */
int het_rows_linear_bias(const int64_t* offsets, const float* x, const float* w, const float* bias, float* out,
                         int64_t num_rows, int64_t K, int64_t X, het_stream stream);
/* ... with bf16 rows: x [*,K] and out [*,X] het_bf16 (x widened on load, out rounded once at the store), w and bias fp32; the bias is
 * added in fp32 BEFORE the rounding.  K and X in {32, 64, 128}, 16-byte aligned tensors (HET_ERR_UNSUPPORTED otherwise). */
int het_rows_linear_bias_bf16(const int64_t* offsets, const het_bf16* x, const float* w, const float* bias, het_bf16* out,
                              int64_t num_rows, int64_t K, int64_t X, het_stream stream);

/* layer epilogue (RGAT/models.py:377-383: h + loop_message + h_bias): out[i,:] = a[i,:] (+ b[i,:]) (+ bias[:]) in one
 * pass; b and bias optional, X % 4 == 0 */
int het_rows_add_bias(const float* a, const float* b, const float* bias, float* out, int64_t num_rows, int64_t X,
                      het_stream stream);

/* Typed LayerNorm over rows (HGT's use_norm, HGT/models_dgl.py:131-138: one LayerNorm(out_dim) per node type after the typed output
 * projection).  Row v of the run t of offsets [T+1] (device array, non-decreasing, offsets[0] = 0, offsets[T] = num_rows) that holds it:
 *   mean_v = SUM_j y[v,j] / X    var_v = SUM_j (y[v,j] - mean_v)^2 / X  (biased, as torch.nn.LayerNorm; two-pass in registers)
 *   out[v,:] = (y[v,:] - mean_v) * rsqrt(var_v + eps) * gamma[t,:] + beta[t,:]          gamma, beta [T,X] fp32
 * Shapes: X % 4 == 0, 4 <= X <= 1024, y / out rows 16-byte aligned (8-byte for the bf16 entries), gamma / beta 16-byte aligned:
 * HET_ERR_UNSUPPORTED otherwise, before any launch (het_rows_layer_norm_ok answers for the width).  Null data pointers are
 * HET_ERR_INVALID_ARG; num_rows == 0 is HET_OK.  Rows outside [0, num_rows) are never touched whatever offsets holds. */
int het_rows_layer_norm_ok(int64_t X);
/* bytes of the backward's workspace (one partial row pair [2,X] per row tile, fp32); -1 for an unsupported width */
int64_t het_rows_layer_norm_backward_workspace_bytes(int64_t num_rows, int64_t num_types, int64_t X);
/* forward: writes out [num_rows,X] and, when both are given, mean / rstd [num_rows] fp32 for the backward (both NULL: an
 * evaluation pass, nothing is saved) */
int het_rows_layer_norm(const int64_t* offsets, int64_t num_types, const float* y, const float* gamma, const float* beta, double eps,
                        float* out, float* mean, float* rstd, int64_t num_rows, int64_t X, het_stream stream);
/* backward, one pass over y, grad_out, mean, rstd: with xhat = (y - mean) * rstd and a = grad_out * gamma[t],
 *   grad_y = rstd * (a - mean_j(a) - xhat * mean_j(a * xhat))                      (grad_y NULL: not wanted)
 *   grad_gamma[t,:] = SUM_v grad_out[v,:] * xhat[v,:]    grad_beta[t,:] = SUM_v grad_out[v,:]     over the rows v of type t
 * The column sums leave the pass as one partial per row tile (workspace) and a second small launch adds a type's partials in a
 * fixed order: no float atomics, the same bits every run.  grad_gamma / grad_beta [T,X] are written whole (zeros for an empty type);
 * num_rows == 0 writes nothing. */
int het_rows_layer_norm_backward(const int64_t* offsets, int64_t num_types, const float* y, const float* gamma, const float* mean,
                                 const float* rstd, const float* grad_out, float* grad_y, float* grad_gamma, float* grad_beta,
                                 void* workspace, int64_t workspace_bytes, int64_t num_rows, int64_t X, het_stream stream);
/* ... with bf16 rows: y, out, grad_out and grad_y het_bf16 (widened on load, each result rounded once, to nearest even, at its
 * store); gamma, beta, mean, rstd, every sum and both parameter gradients fp32 */
int het_rows_layer_norm_bf16(const int64_t* offsets, int64_t num_types, const het_bf16* y, const float* gamma, const float* beta,
                             double eps, het_bf16* out, float* mean, float* rstd, int64_t num_rows, int64_t X, het_stream stream);
int het_rows_layer_norm_backward_bf16(const int64_t* offsets, int64_t num_types, const het_bf16* y, const float* gamma,
                                      const float* mean, const float* rstd, const het_bf16* grad_out, het_bf16* grad_y,
                                      float* grad_gamma, float* grad_beta, void* workspace, int64_t workspace_bytes, int64_t num_rows,
                                      int64_t X, het_stream stream);

/* Halo pack / unpack of the multi-GPU path (no reference counterpart: het_amd/dist.py pushes the features of remote source
 * nodes with an all-to-all before the forward and returns their gradients after the backward).
 *   het_rows_gather:       out[i, :] = x[idx[i], :]        i in [0, num_rows)   (X % 4 == 0, 16-byte aligned rows)
 *   het_rows_scatter_add:  out[idx[i], :] += src[i, :]     (atomic: idx may repeat) */
int het_rows_gather(const float* x, const int64_t* idx, int64_t num_rows, int64_t X, float* out, het_stream stream);
int het_rows_scatter_add(const float* src, const int64_t* idx, int64_t num_rows, int64_t X, float* out, het_stream stream);
/*   het_rows_scatter_add_grouped: the same sum without float atomics (and deterministic) for an idx that is used every step:
 *   by_idx = het_grouping_create(NULL, 0, idx, n, out_rows, payload0 = 0 .. n-1, NULL); X a power of two in 4 .. 256. */
int het_rows_scatter_add_grouped(const het_grouping* by_idx, const float* src, int64_t X, float* out, int64_t out_rows,
                                 het_stream stream);

/* Row-sparse access to a learnable table for sampled mini-batches (no reference counterpart: RGNNUtils.py:78-119 keeps the dense
 * [N, K] table and dense Adam; het_amd/layers.py HET_RelGraphEmbed(sparse=True) + het_amd/optim.py RowSparseAdam).  table / p / m / v
 * are fp32 [num_table_rows, K]; row offsets are 64-bit (num_table_rows * K may pass 2^31).
 * Shapes: K % 4 == 0, 4 <= K <= 1024 (het_rows_embed_ok answers for the width): HET_ERR_UNSUPPORTED otherwise, before any launch.
 * num_rows == 0 is HET_OK without a launch.  Null or misaligned pointers (fp32 tensors 16 bytes, bf16 rows and id lists 8 bytes) are
 * HET_ERR_INVALID_ARG, nothing enqueued.  An id outside [0, num_table_rows) is never dereferenced: the gather writes a row of
 * zeros for it, the Adam step skips it.
 *   het_rows_embed_gather:       out[i, :] = table[rows[i], :]   i in [0, num_rows); rows may repeat
 *   het_rows_embed_gather_bf16:  the same with out het_bf16, rounded to nearest even once, at the store */
int het_rows_embed_ok(int64_t K);
int het_rows_embed_gather(const float* table, const int64_t* rows, int64_t num_rows, int64_t num_table_rows, int64_t K, float* out,
                          het_stream stream);
int het_rows_embed_gather_bf16(const float* table, const int64_t* rows, int64_t num_rows, int64_t num_table_rows, int64_t K,
                               het_bf16* out, het_stream stream);
/* One launch of a lazy Adam step on the rows a sparse gradient names.  rows_sorted [num_rows]: ascending ids, repeats allowed; the
 * gradient row of sorted position j is grad[perm[j], :] (perm [num_rows], a permutation of 0 .. num_rows-1; NULL = the identity);
 * grad fp32 [num_rows, K].  For every run of equal ids, with g the sum of the run's gradient rows in position order:
 *   m = beta1 m + (1 - beta1) g     v = beta2 v + (1 - beta2) g g     p -= lr sqrt(bias_correction2) / bias_correction1 * m / (sqrt(v) + eps)
 * in place -- the rule of torch.optim.SparseAdam (eps is added to sqrt(v) before the bias correction of v, unlike dense Adam; rows the
 * gradient does not name keep p, m and v bit for bit).  bias_correction{1,2} = 1 - beta{1,2}^step, formed by the caller.
 * No atomics: one lane group sums a run in a fixed order, the same bits every launch; correctly rounded sqrt and division. */
int het_rows_adam(float* p, float* m, float* v, const int64_t* rows_sorted, const int64_t* perm, const float* grad, int64_t num_rows,
                  int64_t num_table_rows, int64_t K, double lr, double beta1, double beta2, double eps, double bias_correction1,
                  double bias_correction2, het_stream stream);

/* ------------------------------------------------------------------------
 * Layout builders (the step before the path).  Device-side replacements of the reference's CPU
 * converters: torch.ops.torch_hrt.convert_integrated_{coo,csr}_to_separate_{coo,csr} / transpose_csr
 * (OpExport/DataConverters.inc.h:10-344 over MyHyb/MyHyb.h:1047-1150) and the Python unique-list builders
 * (hrt/python/utils_lite/mydgl_graph_methods.py:10-157).  int64 device arrays in and out, outputs caller-allocated;
 * one stable radix sort per call; the call returns after the stream has drained (temporaries are freed).
 * ------------------------------------------------------------------------ */
/* edges bucketed by relation (out_rel_ptrs [R+1]), inside a bucket sorted by eid (< eid_bound), ties in input order */
int het_layout_separate_coo(const int64_t* row, const int64_t* col, const int64_t* rel, const int64_t* eids,
                            int64_t num_edges, int64_t num_rels, int64_t eid_bound, int64_t* out_rel_ptrs,
                            int64_t* out_row, int64_t* out_col, int64_t* out_eids, het_stream stream);
/* integrated COO -> CSR over `row` (stable); out_row_ptrs [num_rows+1] */
int het_layout_coo_to_csr(const int64_t* row, const int64_t* col, const int64_t* rel, const int64_t* eids,
                          int64_t num_edges, int64_t num_rows, int64_t* out_row_ptrs, int64_t* out_col, int64_t* out_rel,
                          int64_t* out_eids, het_stream stream);
/* transpose_csr: rows of the result are the columns of the input; out_row_ptrs [num_cols+1] */
int het_layout_transpose_csr(const int64_t* row_ptrs, const int64_t* col, const int64_t* eids, const int64_t* rel,
                             int64_t num_rows, int64_t num_edges, int64_t num_cols, int64_t* out_row_ptrs, int64_t* out_col,
                             int64_t* out_eids, int64_t* out_rel, het_stream stream);
/* sorted unique (relation, node) pairs of a relation-bucketed list: out_nodes (capacity E, or 2E with nodes_b),
 * out_rel_ptrs [R+1], out_inverse (optional; [E], or [2E] for the dual list in the reference's order: per relation the
 * entries of nodes_a then those of nodes_b), *out_count (host) = number of pairs */
int het_layout_unique_rel_nodes(const int64_t* rel_ptrs, int64_t num_rels, const int64_t* nodes_a, const int64_t* nodes_b,
                                int64_t num_edges, int64_t num_nodes, int64_t* out_nodes, int64_t* out_rel_ptrs,
                                int64_t* out_inverse, int64_t* out_count, het_stream stream);

/* ------------------------------------------------------------------------
 * Keyed neighbour sampling and block construction for sampled mini-batches (csrc/block_sample.hip; het_amd/sampling.py
 * NeighborSampler(method="keyed"); no reference counterpart: RGNNUtils.py:164-196 samples with DGL on the CPU).
 * The rule, in wrapping uint64 arithmetic, with pos an edge's position in the in-CSR (row_ptrs over destinations):
 *   sm(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 *   stream = sm(seed ^ sm(draw));  key(pos) = sm(stream + pos)
 *   a destination keeps all its in-edges when deg <= fanout or fanout <= 0, else the fanout edges with the smallest (key, pos);
 *   the kept edges are listed destination by destination (the order of dst), in ascending pos inside one.
 * int64 device arrays, caller-allocated outputs.  Before anything is enqueued: negative counts and num_rels < 1 are
 * HET_ERR_INVALID_ARG; num_dst == 0 or total == 0 is HET_OK (the host results are 0); null pointers are HET_ERR_INVALID_ARG.
 * Ids and positions outside their ranges are never turned into addresses.  The device temporaries come from het_set_allocator's
 * allocator and are released in stream order; only the two entries that return a count to the host wait for the stream.
 * ------------------------------------------------------------------------ */
/* in-degree from which het_sample_select gives a destination to a workgroup instead of a wave, and the positions per emission
 * chunk (= threads) of that workgroup */
int het_sample_workgroup_degree(void);
int het_sample_chunk(void);
/* out_offsets [num_dst + 1] = exclusive sum of the kept counts min(deg, fanout) (deg when fanout <= 0); *out_total (host) = the sum */
int het_sample_count(const int64_t* row_ptrs, const int64_t* dst, int64_t num_dst, int64_t num_nodes, int64_t fanout,
                     int64_t* out_offsets, int64_t* out_total, het_stream stream);
/* out_pos / out_owner [total]: in-CSR position and index into dst of every kept edge; offsets / total as het_sample_count gave
 * them for the same row_ptrs, dst and fanout (an offset that would write past total writes nothing).  Reads row_ptrs only. */
int het_sample_select(const int64_t* row_ptrs, const int64_t* dst, int64_t num_dst, int64_t num_nodes, int64_t fanout, int64_t seed,
                      int64_t draw, const int64_t* offsets, int64_t total, int64_t* out_pos, int64_t* out_owner, het_stream stream);
/* Local node ids of a block.  src [num_edges]: the in-CSR's column (source) of every position; dst [num_dst]: DISTINCT node ids;
 * map [num_nodes]: scratch that holds -1 everywhere on entry and again when the enqueued work has run.  out_nodes (capacity
 * num_dst + total) = dst followed by the sampled sources that are no destination, ascending by global id; out_local_src [total] =
 * index into out_nodes of every kept edge's source; *out_num_extra (host) = number of appended nodes.  New nodes are claimed with
 * compare-and-swap in whatever order the hardware runs them and then sorted, so the result does not depend on that order. */
int het_block_renumber(const int64_t* src, int64_t num_edges, const int64_t* pos, int64_t total, const int64_t* dst, int64_t num_dst,
                       int64_t* map, int64_t num_nodes, int64_t* out_nodes, int64_t* out_local_src, int64_t* out_num_extra,
                       het_stream stream);
/* The kept edges relation-major, stable (the order of pos / owner inside a relation): out_rel_ptrs [num_rels + 1], and per block
 * edge out_row = local source, out_col = owner, out_rel = relation, out_eids = eids[pos] (rel / eids [num_edges]: the in-CSR's) */
int het_block_relation_major(const int64_t* rel, const int64_t* eids, int64_t num_edges, const int64_t* pos, const int64_t* owner,
                             const int64_t* local_src, int64_t total, int64_t num_rels, int64_t* out_rel_ptrs, int64_t* out_row,
                             int64_t* out_col, int64_t* out_rel, int64_t* out_eids, het_stream stream);

/* ------------------------------------------------------------------------
 * The ComplEx head for link prediction (csrc/triple_score.hip, csrc/triple_rank.hip; het_amd/linkpred.py ComplExDecoder,
 * complex_rank): the score, its backward and the filtered ranking of the DistMult head (the two sections below, whose
 * triples, plan, lists, chunks, bad ids, counters, workspaces and checks hold here word for word) with another trilinear form, one
 * that tells a triple from its reverse.  (The section stands here because the sections after it are pinned to their neighbours.)
 *   Layout: h [num_nodes, dim] and w [num_rels, dim] with dim even; column 2k is the real and column 2k + 1 the imaginary part of
 *   component k (torch.view_as_complex(x.view(-1, dim / 2, 2))).  A 16-byte piece of a row is two whole complex numbers: the widths
 *   served are those of het_triple_params (score, backward) and het_triple_rank_params (ranking), multiples of 4.
 *   With a = h[s_j], b = w[r_j], c = h[o_j], per component (a_r, a_i), (b_r, b_i), (c_r, c_i), g = grad_score_j:
 *     score_j    = sum_k Re(a_k * b_k * conj(c_k)) = sum_k (a_r b_r - a_i b_i) c_r + (a_r b_i + a_i b_r) c_i
 *     grad a_r  += g (b_r c_r + b_i c_i)      grad a_i += g (b_r c_i - b_i c_r)      (slot side 0: v is the head s_j)
 *     grad c_r  += g (a_r b_r - a_i b_i)      grad c_i += g (a_r b_i + a_i b_r)      (slot side 1: v is the tail o_j)
 *     grad b_r  += g (a_r c_r + a_i c_i)      grad b_i += g (a_r c_i - a_i c_r)
 *   The orders are het_distmult_score_backward's: a node's slots ascending 2 j + side, a list longer than L in chunks of L with the
 *   chunk sums added in chunk order, grad_w in chunks of the relation chunk, every grad_h and grad_w row written exactly once (+0 where
 *   a list is empty), het_bf16 grad_h rounded once after the whole sum, a triple with s_j == o_j has both slots, a bad id is counted
 *   and never forms an address.  No float atomics, no zero-fill, no read-back: the same bits on every call.  The plan is
 *   het_triple_plan's and the backward's workspace holds het_distmult_score_backward_workspace bytes.
 *   het_complex_rank: query j = (anchor [j], rel [j], truth [j], side [j]).  side 0 ranks tails: the anchor is the head s and the
 *   candidates stand in o's place.  side 1 ranks heads: the anchor is the tail o and the candidates stand in s's place.  A side
 *   outside {0, 1} makes the query bad.  With x = h[a_j], b = w[r_j], every operation a separately rounded fp32 one (no fused
 *   multiply-add):
 *     side 0:  q_j[2k] = fl32(fl32(x_r b_r) - fl32(x_i b_i))     q_j[2k+1] = fl32(fl32(x_r b_i) + fl32(x_i b_r))
 *     side 1:  q_j[2k] = fl32(fl32(b_r x_r) + fl32(b_i x_i))     q_j[2k+1] = fl32(fl32(b_r x_i) - fl32(b_i x_r))
 *     score_j(c) = the fp32 fma chain over ascending d from +0: acc = fmaf(q_j[d], h[c, d], acc);  p_j = score_j(t_j) by the same chain
 *   so that score_j(c) is the ComplEx score of (a_j, r_j, c) on side 0 and of (c, r_j, a_j) on side 1.  The run, the exclusions, the
 *   three counters, the bad count, the launches behind the prelude and the workspace (het_triple_rank_workspace) are het_triple_rank's.
 * The checks, codes and messages are those of the DistMult entries, each naming its own entry; a dim that is odd or no multiple of 4
 * is HET_ERR_UNSUPPORTED; het_complex_rank refuses a null or misaligned side (HET_ERR_INVALID_ARG).
 * ------------------------------------------------------------------------ */
int het_complex_score(const float* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples,
                      int64_t num_nodes, int64_t num_rels, int64_t dim, float* score, het_stream stream);
int het_complex_score_bf16(const het_bf16* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples,
                           int64_t num_nodes, int64_t num_rels, int64_t dim, float* score, het_stream stream);
int het_complex_score_backward(const float* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                               const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots, const int64_t* rel_ptr,
                               const int64_t* rel_order, const int64_t* chunk_ptr, int64_t num_triples, int64_t num_nodes, int64_t num_rels,
                               int64_t dim, float* grad_h, float* grad_w, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_complex_score_backward_bf16(const het_bf16* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                                    const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots, const int64_t* rel_ptr,
                                    const int64_t* rel_order, const int64_t* chunk_ptr, int64_t num_triples, int64_t num_nodes,
                                    int64_t num_rels, int64_t dim, het_bf16* grad_h, float* grad_w, void* workspace,
                                    int64_t workspace_bytes, het_stream stream);
int het_complex_rank(const float* h, const float* w, const int64_t* anchor, const int64_t* rel, const int64_t* truth, const int64_t* side,
                     int64_t num_queries, const int64_t* pair_query, const int64_t* pair_cand, int64_t num_pairs,
                     const int64_t* node_type_offsets, int64_t num_types, int64_t num_nodes, int64_t num_rels, int64_t dim, int32_t* greater,
                     int32_t* equal, int32_t* cands, int64_t* bad, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_complex_rank_bf16(const het_bf16* h, const float* w, const int64_t* anchor, const int64_t* rel, const int64_t* truth,
                          const int64_t* side, int64_t num_queries, const int64_t* pair_query, const int64_t* pair_cand, int64_t num_pairs,
                          const int64_t* node_type_offsets, int64_t num_types, int64_t num_nodes, int64_t num_rels, int64_t dim,
                          int32_t* greater, int32_t* equal, int32_t* cands, int64_t* bad, void* workspace, int64_t workspace_bytes,
                          het_stream stream);

/* ------------------------------------------------------------------------
 * Filtered ranking of link-prediction queries with the DistMult score (csrc/triple_rank.hip; het_amd/linkpred.py distmult_rank;
 * DESIGN.md 4.14).  Every query is ranked against every node of its true node's type; no score is stored, three int32 per query
 * come out.  (The section stands here, before keyed dropout, because the sections after it are pinned to their neighbours.)
 *   query j    (a_j, r_j, t_j) = (anchor [j], rel [j], truth [j]): anchor node, relation, true node.  Tail ranking of (s, r, o): a = s,
 *              t = o.  Head ranking: a = o, t = s.  DistMult is symmetric, so one kernel serves both.
 *   run        [lo_j, hi_j) = the run of node_type_offsets [num_types + 1] (DEVICE memory) that holds t_j; NULL: [0, num_nodes)
 *   q_j[d]     = fl32(h[a_j, d] * w[r_j, d])       h [num_nodes, dim] float, or het_bf16 widened on load (exact); w [num_rels, dim] float
 *   score_j(c) = the fp32 fma chain over ascending d, from +0:  acc = fmaf(q_j[d], h[c, d], acc)
 *   p_j        = score_j(t_j), by the same chain
 *   excluded   c == t_j, and every c with a listed pair (pair_query [i], pair_cand [i]) = (j, c), i < num_pairs; a pair listed twice
 *              excludes once; a listed c outside the run changes nothing; a pair with an id outside [0, num_queries) x [0, num_nodes)
 *              is ignored
 *   greater[j] = #{ c in run, not excluded : score_j(c) >  p_j }
 *   equal[j]   = #{ c in run, not excluded : score_j(c) == p_j }
 *   cands[j]   = #{ c in run, not excluded }
 *   bad        a_j or t_j outside [0, num_nodes), r_j outside [0, num_rels), or t_j in no run: counted in bad [1] (int64, device),
 *              not asserted; greater = equal = cands = 0 and no table is read through such an id.
 * The chain is the arithmetic of v_mfma_f32_16x16x4_f32 (one rounding per product, k ascending), which scores the candidates; p_j is
 * a sequential fmaf chain in plain C++: a candidate whose row has the bits of t_j's row ties with it exactly.
 * The counters start at zero by the library's own doing: the prelude launch stores 0 into greater / equal / cands of every query
 * before the rank pass (the next launch on the stream) adds to them with integer atomics, and bad is cleared by an 8-byte
 * hipMemsetAsync before the prelude counts into it.  No float atomic: the same inputs give the same bits on every call.
 * Launches: the memset, the prelude, with pairs a key launch, one stable radix sort of the pairs by tile cell and a launch that
 * finds every candidate tile's run of them, the rank pass.  Nothing is read back and nothing waits for the stream.  The workspace
 * holds het_triple_rank_workspace(num_queries, num_pairs, num_nodes, dim) bytes: q [num_queries, dim] float, p / lo / hi / t
 * [num_queries] 4 bytes each, and with pairs the sort's keys (8 bytes) and values (4 bytes) in and out, 4 bytes per candidate tile
 * plus 4, each part rounded up to 256 bytes, and the sort's own scratch.
 * het_triple_rank_params (out [8] on the host): queries of a tile, candidates of a tile, the least and the greatest dim served (a
 * multiple of 4 between them), threads per workgroup, the most workgroups, the query tiles whose counters a workgroup keeps, the most
 * candidate tiles of one work item.
 * Before anything is enqueued: negative counts, num_queries or num_pairs >= 2^30, num_nodes or num_rels >= 2^31 - 1, dim < 1,
 * node_type_offsets with num_types < 1, a null pointer where the count is positive, a misaligned pointer (h on 16-byte (bf16: 8-byte),
 * w / workspace on 16-byte, int64 arrays on 8-byte, the counts on 4-byte boundaries) and a workspace smaller than its query says are
 * HET_ERR_INVALID_ARG; a dim the kernels do not take is HET_ERR_UNSUPPORTED.  num_queries == 0 is HET_OK with no launch.
 * ------------------------------------------------------------------------ */
int64_t het_triple_rank_workspace(int64_t num_queries, int64_t num_pairs, int64_t num_nodes, int64_t dim); /* bytes; -1 on bad sizes */
int het_triple_rank(const float* h, const float* w, const int64_t* anchor, const int64_t* rel, const int64_t* truth, int64_t num_queries,
                    const int64_t* pair_query, const int64_t* pair_cand, int64_t num_pairs, const int64_t* node_type_offsets,
                    int64_t num_types, int64_t num_nodes, int64_t num_rels, int64_t dim, int32_t* greater, int32_t* equal, int32_t* cands,
                    int64_t* bad, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_triple_rank_bf16(const het_bf16* h, const float* w, const int64_t* anchor, const int64_t* rel, const int64_t* truth,
                         int64_t num_queries, const int64_t* pair_query, const int64_t* pair_cand, int64_t num_pairs,
                         const int64_t* node_type_offsets, int64_t num_types, int64_t num_nodes, int64_t num_rels, int64_t dim,
                         int32_t* greater, int32_t* equal, int32_t* cands, int64_t* bad, void* workspace, int64_t workspace_bytes,
                         het_stream stream);
int het_triple_rank_params(int64_t* out);

/* ------------------------------------------------------------------------
 * Keyed dropout fused with the activation (csrc/keyed_dropout.hip; het_amd/layers.py KeyedDropout; no reference counterpart: the
 * reference's layers end with activation(h) and nn.Dropout).  The mask is a pure function of (seed, draw, position) on the
 * sampler's stream above, recomputed by the backward and never stored.  With i the index in the contiguous tensor of n elements:
 *   T      = min(llround(p * 65536), 65535)              the effective rate is T / 65536 (0.5 is exact)
 *   scale  = (float)(65536.0 / (65536 - T))              computed in double, rounded once to float
 *   stream = sm(seed ^ sm(draw));  key(g) = sm(stream + g),  g = (base + i) / 4: one key per 4 consecutive elements
 *   field  = (key(g) >> (16 * ((base + i) % 4))) & 0xFFFF;   kept(i) = field >= T
 *   a(y)   = y (activation 0: none)  |  y < 0 ? 0 : y (activation 1: relu; a NaN stays a NaN)
 *   out[i]    = kept(i) ? a(y[i]) * scale : +0           (a select, not a multiply: a dropped NaN or inf is +0)
 *   grad_y[i] = kept(i) && (activation == 0 || out[i] > 0) ? grad_out[i] * scale : +0
 * base: the index of the tensor's first element in the stream, a multiple of 4, at least 0 (a mask cut into parts; 0 for a whole
 * tensor).  A tail of n % 4 elements uses the low fields of its group.  bf16 rows are widened (exact), multiplied in fp32 and
 * rounded once, to nearest even, at the store; the fp32 product is one correctly rounded multiply: every output is determined to
 * the bit.  seed and draw are the 64 bits of the rule's unsigned values, passed as int64_t like het_sample_select's.
 * Before anything is enqueued: n < 0, a null pointer, a pointer off a 16-byte (bf16: 8-byte) boundary, base < 0 or base % 4 != 0,
 * p outside [0, 1) or a NaN, and relu's backward without out are HET_ERR_INVALID_ARG; an activation other than 0 / 1 is
 * HET_ERR_UNSUPPORTED; n == 0 is HET_OK with nothing looked at.  out may not overlap y (refused).  grad_y MAY be grad_out itself:
 * every element is read before its own store and no other lane touches it; any other overlap of grad_y is refused.  out is read
 * by the backward for relu only (NULL otherwise).  One launch each, no workspace, no atomics, no host synchronisation.
 * ------------------------------------------------------------------------ */
int het_keyed_dropout(const float* y, float* out, int64_t n, int64_t base, int activation, double p, int64_t seed, int64_t draw,
                      het_stream stream);
int het_keyed_dropout_backward(const float* grad_out, const float* out, float* grad_y, int64_t n, int64_t base, int activation,
                               double p, int64_t seed, int64_t draw, het_stream stream);
int het_keyed_dropout_bf16(const het_bf16* y, het_bf16* out, int64_t n, int64_t base, int activation, double p, int64_t seed,
                           int64_t draw, het_stream stream);
int het_keyed_dropout_backward_bf16(const het_bf16* grad_out, const het_bf16* out, het_bf16* grad_y, int64_t n, int64_t base,
                                    int activation, double p, int64_t seed, int64_t draw, het_stream stream);
/* the rule's T and scale for a rate p in [0, 1) (HET_ERR_INVALID_ARG otherwise, and for a null pointer) */
int het_keyed_dropout_params(double p, uint32_t* T, float* scale);

/* ------------------------------------------------------------------------
 * Link prediction on triples (csrc/triple_score.hip; het_amd/linkpred.py): keyed corruption of positive edges, the
 * inverted index ("plan") of a batch of triples, the DistMult score and its backward.  No entry reads anything back to the host or
 * waits for the stream; no float is added by more than one writer: the same bits on every call.
 *   Triples: p positives (src_i, rel_i, dst_i) and k >= 0 corruptions of each: t = p * (1 + k) triples (s_j, r_j, o_j); j < p is
 *   positive j, j = p + m with m = i * k + c is corruption c of positive i.  The label (1 for j < p, else 0) is the position.
 *   het_triple_corrupt (one launch, reads no table), all key arithmetic in wrapping uint64, sm as for the keyed sampler:
 *     stream = sm(seed ^ sm(draw));  key = sm(stream + m);  side = key >> 63 (0: the tail o is replaced, 1: the head s);
 *     u = (key >> 31) & 0xFFFFFFFF;  v_old = side ? src_i : dst_i;  [lo, hi) = the run of node_type_offsets [num_types + 1] (DEVICE
 *     memory; NULL: [0, num_nodes)) that holds v_old;  v_new = lo + ((u * (hi - lo)) >> 32);  r_j = rel_i.
 *     Unfiltered: v_new == v_old and true edges may be drawn.  An end that lies in no run is copied as it is.
 *   A triple with s or o outside [0, num_nodes) or r outside [0, num_rels) is BAD: counted, its score is +0, it is in no list of the
 *   plan and in no gradient, and no address is formed from its ids.
 *   het_triple_plan: node_ptr [num_nodes + 1], node_slots [2 t] (slot 2 j + side: side 0 is the head s_j, side 1 the tail o_j; ascending
 *     inside a node), rel_ptr [num_rels + 1], rel_order [t] (ascending j inside a relation), chunk_ptr [num_nodes + num_rels + 2] (the
 *     exclusive sums of the chunk counts of the nodes' and then the relations' lists) and bad [1], all int64 on the device; the
 *     workspace holds het_triple_plan_workspace bytes.  num_nodes and num_rels below 2^31 - 1, t below 2^30.
 *   score_j = sum_d h[s_j, d] * w[r_j, d] * h[o_j, d] in fp32: h [num_nodes, dim] float (or het_bf16, widened first: exact), w
 *     [num_rels, dim] float, score [t] float.  One launch.
 *   het_distmult_score_backward, for grad_score [t]:
 *     grad_h[v] = sum over v's slots, ascending, of grad_score_j * w[r_j] (.) h[the other end of j] (a triple with s_j == o_j == v has
 *       two slots); a list longer than L = params[3] slots is summed in chunks of L from its start and the chunk sums are added in
 *       chunk order.  In h's type (het_bf16: rounded once, to nearest even, after the whole sum).
 *     grad_w[r] = sum over r's triples, ascending j in chunks of params[4], of grad_score_j * (h[s_j] (.) h[o_j]); chunk sums in chunk order.
 *     Every row of both is written exactly once, +0 where a list is empty: nothing has to be zero-filled.  grad_h or grad_w NULL: that
 *     gradient is not wanted and its launches are left out.  With t == 0 both are still written (+0) and no plan is read.
 * het_triple_params (out [7] on the host): the least and the greatest dim served (a multiple of 4 between them), the most lanes a
 * triple gets (the power of two G with dim <= 4 * G, at most out[2]), L, the grad_w chunk, the most workgroups, threads per workgroup.
 * Before anything is enqueued: negative counts, dim < 1, a null pointer where the count is positive, a misaligned pointer (h / grad_h
 * on 16-byte (bf16: 8-byte), w / grad_w / workspace on 16-byte, int64 arrays on 8-byte, score / grad_score on 4-byte boundaries), a
 * workspace smaller than its query says and grad_h overlapping h are HET_ERR_INVALID_ARG; a dim the kernels do not take is
 * HET_ERR_UNSUPPORTED.  t == 0 (p == 0) is HET_OK with no launch, but for the backward (above).
 * ------------------------------------------------------------------------ */
int het_triple_corrupt(const int64_t* src, const int64_t* rel, const int64_t* dst, int64_t num_pos, int64_t num_neg, int64_t seed,
                       int64_t draw, const int64_t* node_type_offsets, int64_t num_types, int64_t num_nodes, int64_t* s, int64_t* r,
                       int64_t* o, het_stream stream);
int64_t het_triple_plan_workspace(int64_t num_triples, int64_t num_nodes, int64_t num_rels); /* bytes; -1 (and het_last_error) on bad sizes */
int het_triple_plan(const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples, int64_t num_nodes, int64_t num_rels,
                    int64_t* node_ptr, int64_t* node_slots, int64_t* rel_ptr, int64_t* rel_order, int64_t* chunk_ptr, int64_t* bad,
                    void* workspace, int64_t workspace_bytes, het_stream stream);
int het_distmult_score(const float* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples,
                       int64_t num_nodes, int64_t num_rels, int64_t dim, float* score, het_stream stream);
int het_distmult_score_bf16(const het_bf16* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples,
                            int64_t num_nodes, int64_t num_rels, int64_t dim, float* score, het_stream stream);
int64_t het_distmult_score_backward_workspace(int64_t num_triples, int64_t num_rels, int64_t dim); /* bytes; -1 on bad sizes */
int het_distmult_score_backward(const float* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                                const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots, const int64_t* rel_ptr,
                                const int64_t* rel_order, const int64_t* chunk_ptr, int64_t num_triples, int64_t num_nodes, int64_t num_rels,
                                int64_t dim, float* grad_h, float* grad_w, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_distmult_score_backward_bf16(const het_bf16* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                                     const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots, const int64_t* rel_ptr,
                                     const int64_t* rel_order, const int64_t* chunk_ptr, int64_t num_triples, int64_t num_nodes,
                                     int64_t num_rels, int64_t dim, het_bf16* grad_h, float* grad_w, void* workspace,
                                     int64_t workspace_bytes, het_stream stream);
int het_triple_params(int64_t* out);

/* ------------------------------------------------------------------------
 * Softmax cross-entropy over the rows of [n, c] logits with integer labels (csrc/softmax_xent.hip; het_amd/layers.py
 * SoftmaxCrossEntropy; the reference's scripts call F.cross_entropy / F.nll_loss of torch).  The forward is one launch plus a
 * one-wave finish, the backward one launch; neither reads anything back to the host.
 *   logits [n, c] float (or het_bf16, widened first: exact), contiguous; labels [n] int64.
 *   Row i is VALID when labels[i] != ignore_index and 0 <= labels[i] < c.  Any other row is skipped: it adds nothing to the loss,
 *   its lse is +0 and its gradient row is +0; a skipped row whose label is not ignore_index is counted as BAD.  No address is formed
 *   from a label that has not passed this test (torch asserts on the device instead).
 *   Per valid row, in fp32:  m = max_c z_c;  lse = m + logf(sum_c exp(z_c - m));  loss_i = logf(sum) + (m - z[label]).
 *     A -inf logit adds 0 to the sum; -inf at the label gives +inf; a row of -inf, or one holding a NaN or +inf, has a NaN lse and loss.
 *     exp in the two streaming passes is the hardware's exp2 of x * log2(e): relative error about (|x| + 1) * 2^-23, exact at 0.
 *   correct_i: z[label] is the first of the row's maxima, a NaN ordered above everything (torch.argmax on the CPU).
 *   loss (fp32 scalar) = sum_i loss_i (HET_XENT_SUM) or that / valid (HET_XENT_MEAN; no valid row: NaN).  Every wave adds its rows
 *     in fp64 in a fixed order and stores one partial in the workspace, one wave adds the partials in a fixed order: no float
 *     atomics, the same bits on every call.  stats [3] int64 = (valid, correct, bad), summed the same way (nothing is zero-filled).
 *   lse [n] float, written for the backward; NULL = not wanted (evaluation).
 *   grad_logits[i, j] = (exp(z_j - lse_i) - [j == labels[i]]) * g * (1 | 1 / valid), in the logits' type (het_bf16: rounded once,
 *     to nearest even, at the store); g = *grad_loss and valid = stats[0] are read from DEVICE memory.  Every element of grad_logits
 *     is written: nothing has to be zero-filled.  Nothing of size [n, c] passes from the forward to the backward but the logits.
 * Any c >= 1 is served, rows that are not 16-byte aligned (c = 3 floats) included; het_softmax_xent_params gives the launch constants
 * (out [4] on the host: columns per lane before a row gets another lane, the most lanes a row gets, the most workgroups, threads
 * per workgroup): a row gets the power-of-two number of lanes G with c <= G * out[0], at most out[1].
 * Before anything is enqueued: n < 0, c < 1, a null pointer where n > 0, logits / grad_logits off a 16-byte (bf16: 8-byte) boundary,
 * labels / stats / workspace off an 8-byte one, a workspace smaller than het_softmax_xent_workspace(n, c) bytes and grad_logits
 * overlapping logits are HET_ERR_INVALID_ARG; a reduction other than the two is HET_ERR_UNSUPPORTED.  n == 0 is HET_OK with no
 * launch and nothing written: the caller's loss is +0 (sum) / NaN (mean) and its stats are zeros.
 * ------------------------------------------------------------------------ */
#define HET_XENT_MEAN 0
#define HET_XENT_SUM 1
int64_t het_softmax_xent_workspace(int64_t n, int64_t c); /* bytes; -1 (and het_last_error) for n < 0 or c < 1 */
int het_softmax_xent(const float* logits, const int64_t* labels, int64_t n, int64_t c, int64_t ignore_index, int reduction, float* loss,
                     float* lse, int64_t* stats, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_softmax_xent_bf16(const het_bf16* logits, const int64_t* labels, int64_t n, int64_t c, int64_t ignore_index, int reduction,
                          float* loss, float* lse, int64_t* stats, void* workspace, int64_t workspace_bytes, het_stream stream);
int het_softmax_xent_backward(const float* logits, const int64_t* labels, const float* lse, const int64_t* stats, const float* grad_loss,
                              int64_t n, int64_t c, int64_t ignore_index, int reduction, float* grad_logits, het_stream stream);
int het_softmax_xent_backward_bf16(const het_bf16* logits, const int64_t* labels, const float* lse, const int64_t* stats,
                                   const float* grad_loss, int64_t n, int64_t c, int64_t ignore_index, int reduction,
                                   het_bf16* grad_logits, het_stream stream);
int het_softmax_xent_params(int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* HET_AMD_H */
