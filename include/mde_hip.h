/*
 * mde_hip.h -- C ABI of libmde_hip.so, the MI355X (gfx950 / CDNA4) implementation of
 * the minimum-distortion-embedding hot path.
 *
 * Every entry point below replaces one seam of the reference (cvxgrp/pymde v0.2.1); the
 * reference location it stands in for is cited as  [ref: file:line].  The reference has
 * no native boundary of its own on this path (it is torch ops called from Python), so
 * this header IS the FFI a maintainer binds with ctypes -- see INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross the boundary.
 *   - Every `*_dev` / unqualified data pointer is a DEVICE pointer on the device that
 *     is current on the calling thread.  `mde_func`, `mde_lbfgs_coef` are HOST structs.
 *   - All work is enqueued asynchronously on `stream` (a hipStream_t passed as void*);
 *     nothing synchronises unless documented ("SYNC").
 *   - The library borrows caller memory for the duration of the enqueued work and never
 *     frees it.  Objects created here (mde_plan, mde_lbfgs) own their device memory.
 *   - Return value: MDE_OK (0) or a negative MDE_E_* code.  No exceptions cross the ABI.
 *     mde_last_error() returns a thread-local human-readable message for the last failure.
 *   - Embeddings / gradients are contiguous row-major float32 [n, d].  Edge lists are
 *     int64 [p, 2] at the boundary (the reference's dtype, problem.py:130-132) and int32
 *     inside a plan.
 */
#ifndef MDE_HIP_H_
#define MDE_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDE_ABI_VERSION 2   /* 2 (round 6): mde_func.e0 / e1, mde_plan_ring_info */

/* ------------------------------------------------------------------ error codes */
#define MDE_OK 0
#define MDE_E_INVALID (-1)     /* bad argument (null pointer, negative size, d out of range) */
#define MDE_E_SELF_EDGE (-2)   /* an edge (i, i) was found        [ref: problem.py:134-140]  */
#define MDE_E_RANGE (-3)       /* an endpoint is outside [0, n)                              */
#define MDE_E_TOO_LARGE (-4)   /* n >= 2^31 or 2p >= 2^31 (int32 plan)                       */
#define MDE_E_HIP (-5)         /* a HIP runtime call failed; see mde_last_error()            */
#define MDE_E_UNSUPPORTED (-6) /* function kind / dimension not handled by the fused path    */

const char* mde_last_error(void);
int mde_abi_version(void);

/* ------------------------------------------------------------------ distortion functions
 * The per-edge distortion f_k(d_k) and its derivative are evaluated inside the kernels.
 * `kind` selects the closed form; `a0` / `a1` are the per-edge parameter arrays
 * (weights w_k for penalties, deviations delta_k for losses; a1 = weights of the
 * weighted losses); s0..s2 are the scalar hyper-parameters.
 * [ref: pymde/functions/penalties.py:112-400, pymde/functions/losses.py:61-239]
 *
 *   penalties (a0 = w)                          s0          s1      s2
 *   MDE_F_LINEAR            w d
 *   MDE_F_QUADRATIC         w d^2
 *   MDE_F_CUBIC             w d^3
 *   MDE_F_POWER             w d^e                e
 *   MDE_F_HUBER             w d^2/2 | w t(d-t/2) t (threshold)     (strict <, :230)
 *   MDE_F_LOGISTIC          w log(1+exp(a(d-t))) t          a
 *   MDE_F_SIGMOID           w sigmoid(a(d-t))    t          a
 *   MDE_F_HINGE             max(0,w(d-(t-sgn(w)s))) t       s (sigma)
 *   MDE_F_LOG1P             w log1p(d^e)         e
 *   MDE_F_LOG               w log(-expm1(-d^e))  e
 *   MDE_F_INVPOWER          |w| / d^e            e
 *   MDE_F_LOGRATIO          w log(d^e/(1+d^e))   e
 *   MDE_F_DEADZONE_QUADRATIC  w (d<t ? 0 : d^2)  t
 *   MDE_F_DEADZONE_CUBIC      w (d<t ? 0 : d^3)  t
 *   MDE_F_CLIPPED_QUADRATIC   w min(d^2,(t+1)^2) t
 *   losses (a0 = delta, r = |delta - d|)
 *   MDE_F_L_QUADRATIC       (delta-d)^2
 *   MDE_F_L_WEIGHTED_QUADRATIC  a1 (delta-d)^2
 *   MDE_F_L_HUBER           r^2 | t(2r-t)        t                   (strict <, losses.py:122)
 *   MDE_F_L_CUBIC           r^3
 *   MDE_F_L_POWER           r^e                  e
 *   MDE_F_L_WEIGHTED_POWER  a1 r^e               e
 *   MDE_F_L_ABSOLUTE        r
 *   MDE_F_L_LOGISTIC        log(1+exp(r))
 *   MDE_F_L_FRACTIONAL      max(delta/d, d/delta) - 1
 *   MDE_F_L_SOFT_FRACTIONAL (1/g)(lse(g delta/d, g d/delta) - log 2 - g)   s0 = g (gamma)
 *   MDE_F_L_CLIPPED_QUADRATIC   min((delta-d)^2,(t+1)^2)  t
 *   MDE_F_L_LOG1P               log(1 + (d-delta)^e)      e   (losses._Log1p; torch.pow semantics:
 *                               NaN for d < delta unless e is an integer)
 *
 * PushAndPull [ref: penalties.py:372-400]: set `kind` to the attractive penalty and
 * `kind_neg` to the repulsive one (with its scalars in n0..n2); an edge uses `kind` when
 * w_k >= 0 and `kind_neg` when w_k < 0 (zero weight is attractive, penalties.py:390).
 * kind_neg = MDE_F_NONE means a plain (single) function.
 */
enum {
  MDE_F_NONE = 0,
  MDE_F_LINEAR = 1,
  MDE_F_QUADRATIC = 2,
  MDE_F_CUBIC = 3,
  MDE_F_POWER = 4,
  MDE_F_HUBER = 5,
  MDE_F_LOGISTIC = 6,
  MDE_F_SIGMOID = 7,
  MDE_F_HINGE = 8,
  MDE_F_LOG1P = 9,
  MDE_F_LOG = 10,
  MDE_F_INVPOWER = 11,
  MDE_F_LOGRATIO = 12,
  MDE_F_DEADZONE_QUADRATIC = 13,
  MDE_F_DEADZONE_CUBIC = 14,
  MDE_F_CLIPPED_QUADRATIC = 15,
  MDE_F_L_QUADRATIC = 32,
  MDE_F_L_WEIGHTED_QUADRATIC = 33,
  MDE_F_L_HUBER = 34,
  MDE_F_L_CUBIC = 35,
  MDE_F_L_POWER = 36,
  MDE_F_L_WEIGHTED_POWER = 37,
  MDE_F_L_ABSOLUTE = 38,
  MDE_F_L_LOGISTIC = 39,
  MDE_F_L_FRACTIONAL = 40,
  MDE_F_L_SOFT_FRACTIONAL = 41,
  MDE_F_L_CLIPPED_QUADRATIC = 42,
  MDE_F_L_LOG1P = 43
};

typedef struct mde_func {
  int32_t kind;      /* MDE_F_* (attractive branch for PushAndPull)                       */
  int32_t kind_neg;  /* MDE_F_NONE, or the repulsive branch of a PushAndPull              */
  const float* a0;   /* device; per-edge weights / deviations.  Order: see each call      */
  const float* a1;   /* device; second per-edge array (weighted losses) or NULL           */
  int32_t a0_scalar; /* 1: a0 points at ONE value broadcast to every edge (nelement()==1);
                        2: a0 is a codebook stream written by mde_plan_expand_codebook (layout 1);
                        3: a0 is a byte-index stream written by mde_plan_expand_bytes (layout 1);
                        4: a0 is a PAIR codebook stream written by mde_plan_expand_codebook_for (layout 1):
                           one or two distinct values, selected by bit 0 of the packed word             */
  int32_t a1_scalar;
  float s0, s1, s2;  /* scalars of `kind`                                                 */
  float n0, n1, n2;  /* scalars of `kind_neg`                                             */
  int32_t layout;    /* order of a0/a1 for mde_average_distortion: 0 = CSR plan order,
                        1 = LDS-ring order (mde_plan_layout / mde_plan_expand_layout)        */
  const float* e0;   /* device; the per-edge arrays behind a0 / a1 in the CALLER'S edge order [p] (the   */
  const float* e1;   /* order of the edge list given to mde_plan_create), or NULL.  Needed with layout 1
                        when the plan's ring layout peels hub rows off to the CSR hub kernel
                        (mde_plan_ring_info: those rows read their parameters through the plan's edge
                        ids); ignored otherwise, and for parameters that are one broadcast scalar    */
} mde_func;

/* ------------------------------------------------------------------ the edge plan
 * One-time device preprocessing of an edge list [ref: problem.py:129-170, the `edges`,
 * `_lhs`, `_rhs` buffers].  The plan stores the SYMMETRISED incidence structure in CSR
 * form: for every vertex v in [row_lo, row_hi) the list of its incident half-edges
 * (neighbour u, original edge id k), so the gradient row of v is a pure gather
 *      grad[v] = sum_{h in row v} g_h (x_v - x_{nbr[h]})
 * with no atomics and a fixed summation order (bitwise reproducible).  Half-edges of a
 * row keep the order of their original edge ids (stable sort).
 *
 * row_lo/row_hi select the vertex range this plan (rank) owns; pass 0, n for a
 * single-GPU plan.  Validation (self edges, range) always covers the full edge list.
 * SYNC: returns after the plan is built (it must read back counts).
 */
typedef struct mde_plan mde_plan;

int mde_plan_create(int64_t n, int64_t p, const int64_t* edges, int64_t row_lo, int64_t row_hi,
                    void* stream, mde_plan** out);
int mde_plan_destroy(mde_plan* plan);
int64_t mde_plan_n(const mde_plan* plan);
int64_t mde_plan_p(const mde_plan* plan);           /* edges in the full problem           */
int64_t mde_plan_half_edges(const mde_plan* plan);  /* half-edges stored (= 2p if full)    */
int64_t mde_plan_row_lo(const mde_plan* plan);
int64_t mde_plan_row_hi(const mde_plan* plan);
const int32_t* mde_plan_rowptr(const mde_plan* plan); /* [row_hi-row_lo+1], offsets into nbr */
const int32_t* mde_plan_nbr(const mde_plan* plan);    /* [half_edges] neighbour vertex      */
const int32_t* mde_plan_eid(const mde_plan* plan);    /* [half_edges] original edge id      */

/* Copy the plan arrays into caller buffers (rowptr [nloc+1], nbr [H], eid [H]; any may be NULL). */
int mde_plan_export(const mde_plan* plan, int32_t* rowptr_out, int32_t* nbr_out, int32_t* eid_out,
                    void* stream);

/* Balanced vertex-range boundaries for `world` ranks: bounds[r]..bounds[r+1] holds about
 * 2p/world half-edges.  `bounds_host` is a HOST array of world+1 int64.  SYNC. */
int mde_shard_bounds(int64_t n, int64_t p, const int64_t* edges, int32_t world,
                     int64_t* bounds_host, void* stream);

/* out_half[h] = in_edge[eid[h]] : put a per-edge parameter array into plan (CSR) order. */
int mde_plan_expand(const mde_plan* plan, const float* in_edge, float* out_half, void* stream);

/* Layout the fused kernel prefers for embedding dimension d: 0 = the CSR order above,
 * 1 = the LDS-ring layout of mde_ring.hip (d <= 4, embedding table larger than L2: per-wave streams
 * of packed half-edges, chunk-major; built on first request, SYNC).
 * Per-edge parameters for layout 1 are permuted with mde_plan_expand_layout and flagged with
 * mde_func.layout = 1.  Negative return: error. */
int mde_plan_layout(mde_plan* plan, int32_t d, void* stream);
/* Tell the plan which distortion function its next layout decision is for (mde_func.kind / kind_neg): for problems
 * whose table fits L2 and that have fewer than 16 M half-edges the choice between the two layouts is close, and the
 * ring kernel pays for an expensive function (PushAndPull, Log, the run-time functor of private kinds) where the CSR
 * kernels hide it behind their gathers.  Optional (default: a Log1p-class function); call it before mde_plan_layout.
 * Never changes a result, only which kernel computes it. */
int mde_plan_function_hint(mde_plan* plan, int32_t kind, int32_t kind_neg);
/* Entries of a per-half-edge parameter array in `layout` (layout 1 stores whole 64-entry wave
 * iterations, padded where a stream ends or its chunk window closes, so it is larger than
 * mde_plan_half_edges). */
int64_t mde_plan_layout_half_edges(const mde_plan* plan, int32_t layout);
/* Parameter codebook for layout 1 at d = 2 and d = 3: when `in_edge` [p] holds at most 7 (d = 2) / 3
 * (d = 3) distinct values (k-NN weights 1 / 2, -1 for repulsive pairs, ...) write to out_half
 * [mde_plan_layout_half_edges(plan, 1)] the packed half-edge words with the value index in the low
 * bits their row address leaves free (3 / 2), followed by the 8-entry value table (entry 0 = 0.0, the weight of padding lanes;
 * entries 1..7 the values in ascending bit order), and set *n_values_host to the number of values;
 * the fused kernel then streams 4 instead of 8 bytes per half-edge (mde_func.a0 = out_half,
 * a0_scalar = 2).  *n_values_host = 0: not applicable, nothing written -- use
 * mde_plan_expand_layout (also when a value is NaN or infinite: the kernel skips the NaN/Inf -> 1
 * fix-up of f'/d for codebook streams).  Results are identical either way.  SYNC. */
int mde_plan_expand_codebook(const mde_plan* plan, const float* in_edge, float* out_half,
                             int32_t* n_values_host, void* stream);
/* The same for the function the stream is meant for, which allows a second form.  *form_host receives the value
 * for mde_func.a0_scalar (0 with *n_values_host = 0):
 *   2  the codebook above;
 *   4  the pair codebook, taken when `in_edge` holds ONE or TWO distinct values (unit weights, the {1, 2} of a
 *      neighbour graph) and `f` is a function whose entries with coinciding ends add exactly zero for every finite
 *      parameter (Log1p with exponent 1, 1.5 or 2).  The value table starts with the two values (one value: twice),
 *      the index is bit 0 of the packed word, and the kernel selects between two registers instead of reading the
 *      table from LDS.  Padding entries select entry 0, a real weight: their column field is rewritten to their own
 *      (dummy, zero) row, so their distance is 0.  The stream fits `f` only (kind, kind_neg and s0 are read;
 *      a0 need not be set yet).  MDE_CODEBOOK_PAIR=0 in the environment: always form 2.
 * Results are bitwise identical between the two forms.  SYNC. */
int mde_plan_expand_codebook_for(const mde_plan* plan, const mde_func* f, const float* in_edge, float* out_half,
                                 int32_t* n_values_host, int32_t* form_host, void* stream);
/* Byte-index parameter stream for layout 1 at d = 2 and d = 3: when `in_edge` [p] holds at most 255 distinct
 * values (the hop-count deviations of preserve_distances on a graph [ref: pymde/recipes.py:194-215,
 * preprocess/graph.py:402-474], quantised weights) write to out_half [mde_plan_layout_half_edges(plan, 1)
 * floats of space] one index BYTE per entry of the layout (in the order of the packed half-edge words),
 * followed at byte offset H by the 256-entry value table (entry 0 = 0.0, the weight of padding lanes; entries
 * 1..n the values in ascending bit order), and set *n_values_host = n; the fused kernel then streams 5 instead
 * of 8 bytes per half-edge and keeps the table in LDS (mde_func.a0 = out_half, a0_scalar = 3).
 * *n_values_host = 0: not applicable (more values, a NaN / infinite / > 1e6 value, a layout without 1 KB of LDS
 * behind its chunk ring) -- use mde_plan_expand_layout.  Results are identical either way.  SYNC. */
int mde_plan_expand_bytes(const mde_plan* plan, const float* in_edge, float* out_half,
                          int32_t* n_values_host, void* stream);
int mde_plan_expand_layout(const mde_plan* plan, int32_t layout, const float* in_edge,
                           float* out_half, void* stream);
/* What the LDS-ring layout of the plan looks like (after mde_plan_layout returned 1), 16 HOST int64:
 * [0] built (0 / 1), [1] embedding dimension, [2] rows (LDS slots) per row block, [3] row blocks, [4] column groups,
 * [5] chunks, [6] ring slots, [7] wave iterations, [8] half-edges in the ring streams, [9] padded entries,
 * [10] row blocks PERMUTED (rows dealt to the blocks by degree; every entry adds f / 2), [11] hub rows PEELED off to
 * the CSR hub kernel, [12] their half-edges, [13] their segments, [14] loss band in vertices (below; 0: the entry
 * whose row is the smaller vertex adds an edge's loss term), [15] reserved (0). */
int mde_plan_ring_info(const mde_plan* plan, int64_t* info_host);
/* How the loss terms are spread over the LDS-ring layout, 8 HOST doubles.  Every edge has two entries (one per
 * endpoint) and one of them adds the loss term.  With a loss band of W vertices (d = 2, full plans, rows not permuted)
 * entry (row v, column u) adds it iff (v < u) xor ((v / W + u / W) odd), which gives every workgroup about half of its
 * entries' terms; W = 0: iff v < u.  [0] W, [1] .. [3] blocks of four wave iterations in which no entry / every entry /
 * some entries (per-lane test) add their term, [4], [5] smallest and largest fraction of a workgroup's entries that add
 * their term, [6], [7] reserved (0).  All zero when no layout is built. */
int mde_plan_ring_loss_balance(const mde_plan* plan, double* out_host);
/* Checks the LDS-ring layout on the device, 8 HOST int64.  The lane-stable pairs: out_host[0] = entries of a pair's
 * second wave iteration whose row the first iteration holds on another lane (0 in every layout the builder emits: the
 * kernel reads both accumulators of a pair before it writes either), [1] = rows held by both iterations of a pair,
 * [2] = pairs.  Who adds an edge's loss term (layouts whose rows are not permuted; hub rows included): [3] = edges
 * whose term is not added exactly once over their two entries, as the kernels decide it (0 in every layout the builder
 * emits), [4] = entries whose flag in the packed word (d = 2) disagrees with the rule recomputed from row and column
 * (0 likewise), [5] = edges with both entries in this plan, [6], [7] reserved (0).  All zero when no layout is built.
 * SYNC. */
int mde_plan_ring_check(const mde_plan* plan, int64_t* out_host, void* stream);
/* Processing order of the plan's rows for the general-d kernel (d = 5 .. 512; round 6).  The reference evaluates
 * the edges in the caller's order whatever the numbering of the items [ref: pymde/average_distortion.py:62-106]; here
 * the rows of X gathered at the same time share the caches only when neighbours are close in the order the rows are
 * evaluated in.  The call runs a breadth-first search over the plan's rows and sorts them by (level, row id); nothing
 * is renumbered -- X, the gradient and the plan arrays keep the caller's numbering, results are identical with and
 * without an order.  mode 1: keep the order when the mean distance between the positions of an edge's two ends at
 * least halves; 2: keep it regardless; 0: drop it.  mde_average_distortion calls it with mode 1 on a plan's first
 * evaluation at such a d (env MDE_ROW_ORDER=0 / 2 overrides).  info_host (may be NULL): 4 HOST doubles --
 * [0] an order is in use, [1] mean |v - u| over the local half-edges in the caller's numbering, [2] the same in the
 * order built (0: the search was abandoned -- a level held more than an eighth of the rows, or more than 256
 * components), [3] breadth-first levels.  SYNC; one launch and one 4-byte read-back per level. */
int mde_plan_row_order(mde_plan* plan, int32_t mode, void* stream, double* info_host);
/* dst[0] (DEVICE double) <- the loss the plan's last mde_average_distortion wrote to loss_out, in double, before the
 * rounding to float.  A solve whose rows are sharded across ranks sums the ranks' shares in double and rounds once,
 * like the single-GPU kernel does (the reference's line search branches on the last bit of the loss).  ASYNC. */
int mde_plan_loss_double(const mde_plan* plan, double* dst, void* stream);

/* ------------------------------------------------------------------ edge-list preprocessing
 *  [ref: pymde/preprocess/preprocess.py:11-129]
 * De-duplicate an edge list: rows are put in (min, max) order and the unique rows are written to
 * edges_out [>= p, 2] sorted by (i, j) -- np.unique(axis=0)'s order; *count_host = their number.  An item
 * outside [0, n) is MDE_E_INVALID with a message naming the first such row (here, in mde_edges_count_unique and
 * in the `exclude` list of mde_sample_edges): its key min * n + max would be another edge's.  SYNC. */
int mde_edges_deduplicate(int64_t n, int64_t p, const int64_t* edges, int64_t* edges_out,
                          int64_t* count_host, void* stream);
/* Unique edges (i < j, sorted) with their multiplicity as a float weight; rows with i == j or an
 * item equal to -1 (an empty slot) are dropped, any other item outside [0, n) is MDE_E_INVALID.  This is how the k-NN graph gets weight 2 on mutual neighbours
 * [ref: preprocess/data_matrix.py:141-178, graph.py:51-72].  SYNC. */
int mde_edges_count_unique(int64_t n, int64_t p, const int64_t* edges, int64_t* edges_out,
                           float* weights_out, int64_t* count_host, void* stream);
/* Exact k nearest neighbours (Euclidean) of every row of data [n, nf]
 * [ref: preprocess/data_matrix.py:91-140].  idx_out [n, k] int32 (self excluded; -1 when fewer than
 * k other rows exist), d2_out [n, k] squared distances ascending per row; 1 <= k <= 64;
 * sqn_work: n floats of scratch.  The Gram tiles run on the f32 matrix cores. */
int mde_knn(int64_t n, int32_t nf, const float* data, int32_t k, int32_t* idx_out, float* d2_out,
            float* sqn_work, void* stream);
/* out[r] = |data[r]|^2 for the rows of data [n, nf] (f32; the norms mde_knn forms internally). */
int mde_row_sqnorm(int64_t n, int32_t nf, const float* data, float* out, void* stream);
/* Column statistics of data [n, nf] for the translation that precedes a Euclidean search:
 * stats_out double [2, nf] on the device = (column means, population variances), summed in double without
 * floating-point atomics (the same on every run); bad_row_out int32 [1] on the device = the first row that
 * holds a NaN or an infinity, INT32_MAX when there is none (the statistics mean nothing otherwise).  work:
 * mde_col_stats_work_bytes(n, nf) bytes of scratch (at most 64 MiB); the call allocates nothing.  stats_out
 * and work both NULL: the non-finite scan alone.  ASYNC. */
int64_t mde_col_stats_work_bytes(int64_t n, int32_t nf);
int mde_col_stats(int64_t n, int32_t nf, const float* data, double* stats_out, int32_t* bad_row_out, void* work,
                  void* stream);
/* out [n, nf] = data - mu, mu double [nf] on the device: subtracted in double, rounded to f32 once.  ASYNC. */
int mde_rows_subtract(int64_t n, int32_t nf, const float* data, const double* mu, float* out, void* stream);
/* Exact k nearest rows of a corpus C [n_c, nf] for every row of Q [n_q, nf] (both float32, row-major, on
 * the device): the query-against-corpus form of mde_knn.  idx_out [n_q, k] int32 holds
 * rows of C, -1 where n_c < k; d2_out [n_q, k] the squared Euclidean distances, clamped at 0.  Each row is
 * ordered by (d2, index): ties go to the smaller corpus index.  Nothing is excluded as "self": a query equal
 * to a corpus row lists it at distance 0.  1 <= k <= 64; n_q, n_c < 2^31.
 * The grid is (query block of 64 rows, corpus slice): a workgroup scans only its slice (a whole number of
 * 64-column tiles; the last slices may be shorter or empty) and writes its sorted partial list to scratch
 * [slices, n_q, k]; a second kernel merges the lists of each row by (d2, index).  No atomics.  A distance
 * does not depend on the slice that computed it, so the result is bit-identical for every slice count.
 * slices == 1: the search writes the outputs directly (no list scratch, no merge launch); slices == 0:
 * chosen from the device's CU count (1 when the query blocks alone fill the device, otherwise about four
 * workgroups per CU with at least 16 tiles per slice); 0 <= slices <= 65535.
 * work: caller-allocated scratch of mde_knn_cross_work_bytes(n_q, n_c, k, slices) bytes (the row norms of Q
 * and C, then the partial lists when there is more than one slice); the call allocates nothing.
 * Arguments are checked on the host before any launch: MDE_E_INVALID with a message.
 * mde_knn_cross_work_bytes returns a negative MDE_E_* code for invalid arguments (and, with slices == 0,
 * when no device can be asked for its CU count). */
int64_t mde_knn_cross_work_bytes(int64_t n_q, int64_t n_c, int32_t k, int32_t slices);
int mde_knn_cross(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t k,
                  int32_t slices, int32_t* idx_out, float* d2_out, void* work, void* stream);
/* The nearest pair of rows between every two groups of X [n, nf] (float32, row-major, on the device;
 * csrc/mde_group_nearest.hip).  labels int32 [n] on the device names the group of every row, a
 * value of [0, groups); the labels are the caller's contract and are not checked on the host -- a row whose label lies
 * outside that range belongs to no group and is never read.  2 <= groups <= 1024, 1 <= n < 2^31.
 * d2_out float32 [groups, groups] and row_out int32 [groups, groups]: for A != B, d2_out[A][B] = d2_out[B][A] is the
 * smallest squared distance between a row a of group A and a row b of group B, row_out[A][B] is the row of group A
 * in that pair and row_out[B][A] the row of group B.  With A < B, d2(a, b) is the float32 value mde_knn_cross gives
 * query a against corpus row b, bit for bit, and the minimum is taken under the key (d2, a, b): ties go to the smaller
 * a, then the smaller b, so the result is a function of the input alone.  The diagonal, and the row and column of a
 * group without rows, hold FLT_MAX and -1.
 * The rows are ordered by label and read through that row map; blocks of at most 64 rows never straddle a label, a
 * workgroup (query block, slice) forms only the tiles whose candidate label is above its own -- no same-group tile,
 * no symmetric half -- and keeps one candidate per label; a second kernel folds the blocks and slices in a fixed
 * order.  No atomics: the same bits on every run and for every slice count (slices as in mde_knn_cross, 0: automatic).
 * work: mde_group_nearest_work_bytes(n, groups, slices) bytes of scratch (norms, the row map and its sort arrays, the
 * block table, 12 bytes per (slice, block, group) of partials); the radix sort's own temporary is allocated by the
 * call.  Arguments are checked on the host before any launch: MDE_E_INVALID with a message.  SYNC. */
int64_t mde_group_nearest_work_bytes(int64_t n, int32_t groups, int32_t slices);
int mde_group_nearest(int64_t n, int32_t nf, const float* X, const int32_t* labels, int32_t groups, int32_t slices,
                      float* d2_out, int32_t* row_out, void* work, void* stream);
/* The two-stage Euclidean search (csrc/mde_knn_bf16.hip): every pair of a row of Q [n_q, nf]
 * and a row of C [n_c, nf] (float32, row-major, on the device) is ranked by a bf16 Gram product on the bf16
 * matrix cores, every query keeps a shortlist of its n_cand best by (bf16 d2, index), and the shortlist is
 * re-ranked with the float32 squared distance of mde_knn / mde_knn_cross: a returned pair's d2 has the bits
 * those kernels give it, and when the true k nearest are all on the shortlist the result is theirs.
 * The bf16 copies are of the rows minus mu (double [nf] on the device, one vector for Q and C, subtracted in
 * double; NULL: the rows as given) and serve the shortlist only; the re-rank reads Q and C themselves.
 * self != 0: Q == C and n_q == n_c (the self-join), and a row does not list itself.
 * Outputs as for mde_knn_cross: idx_out [n_q, k] int32 (-1 in the slots beyond the rows available), d2_out
 * [n_q, k], each row ordered by (d2, index).  1 <= k <= n_cand <= 64; n_q, n_c < 2^31.
 * slices: the corpus split of the shortlist kernel, as in mde_knn_cross but in 128-row query blocks and
 * 128-column tiles (0: automatic); the shortlist, and so the result, is identical for every split.
 * work: mde_knn_bf16_work_bytes(...) bytes of scratch (the bf16 copies at a row stride of nf rounded up to
 * 32, four vectors of norms, the shortlist and the per-slice lists); the call allocates nothing.  Arguments are
 * checked on the host before any launch: MDE_E_INVALID with a message.  ASYNC. */
int64_t mde_knn_bf16_work_bytes(int64_t n_q, int64_t n_c, int32_t nf, int32_t k, int32_t n_cand, int32_t slices);
int mde_knn_bf16(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, const double* mu,
                 int32_t self, int32_t k, int32_t n_cand, int32_t slices, int32_t* idx_out, float* d2_out,
                 void* work, void* stream);
/* Ranks of listed corpus rows (csrc/mde_knn_rank.hip): for every row i of Q [n_q, nf] and every
 * entry j = idx[i][c] of its list idx [n_q, m] (int32 rows of C [n_c, nf]; float32, row-major, on the device),
 * rank_out[i][c] = the number of rows l of C with (d2(i, l), l) < (d2(i, j), j) in lexicographic order: 0-based,
 * the nearest row has rank 0 and ties go to the smaller index, the order every k-NN kernel lists by.  d2 is the
 * float32 squared distance of mde_knn / mde_knn_cross / mde_knn_bf16, bit for bit, so the ranks of those
 * kernels' own lists are 0, 1, ..., k - 1 in every row, duplicate rows and every other tie included.
 * self != 0: Q == C and n_q == n_c (the self-join); row i itself is not counted, and an entry equal to i is not
 * ranked.  Entries that are not ranked get rank -1 and d2 FLT_MAX: a negative entry, an entry >= n_c (the
 * entries live on the device and are not checked on the host; no row is read for them), and with self the row
 * itself.  d2_out [n_q, m] (may be NULL) receives d2(i, idx[i][c]).  1 <= m <= 64; n_q, n_c < 2^31.
 * Three launches, no atomics: the thresholds d2(i, j) by the chain of the bf16 search's re-rank; one pass of the
 * 64x64 Gram tile on the grid of mde_knn_cross (query block, corpus slice) in which every query row counts the
 * distances that precede each threshold, written to scratch [slices, n_q, m]; a sum over the slices.  Integer
 * sums: rank_out is identical for every slice count and on every run.  slices as in mde_knn_cross (0: automatic;
 * 1: the counts go to rank_out directly and the third launch is dropped; 0 <= slices <= 65535).
 * work: mde_knn_ranks_work_bytes(n_q, n_c, m, slices) bytes of scratch (the row norms of Q and C, the thresholds
 * and their checked indices, the per-slice counts when there is more than one slice); the call allocates
 * nothing.  Arguments are checked on the host before any launch: MDE_E_INVALID with a message.
 * mde_knn_ranks_work_bytes returns a negative MDE_E_* code for invalid arguments (and, with slices == 0, when no
 * device can be asked for its CU count).  ASYNC. */
int64_t mde_knn_ranks_work_bytes(int64_t n_q, int64_t n_c, int32_t m, int32_t slices);
int mde_knn_ranks(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t self, int32_t m,
                  const int32_t* idx, int32_t slices, int32_t* rank_out, float* d2_out, void* work, void* stream);
/* count_out[i] (int32 [n]) = the number of entries of row i of a [n, ka] that are >= 0 and occur in row i of
 * b [n, kb] (int32 neighbour lists on the device; 1 <= ka, kb <= 64): the size of the intersection of two
 * neighbour lists, an entry that a lists twice counted twice.  ASYNC. */
int mde_knn_list_overlap(int64_t n, int32_t ka, const int32_t* a, int32_t kb, const int32_t* b, int32_t* count_out,
                         void* stream);
/* Sums over all pairs of the distances in two spaces (csrc/mde_pair_moments.hip): what the
 * stress, the distance correlation and the Shepard histogram of pymde_amd.quality are computed from.
 * A [n, nfa] and B [n, nfb] (float32, row-major, on the device) hold the same n rows in two spaces; q_rows int32
 * [n_q] on the device lists the query rows (NULL: all n rows in order, n_q == n; an entry outside [0, n) is the
 * caller's error and is not checked).  For every query i = q_rows[r] and every row j != i (by index: a duplicate of
 * row i elsewhere counts) D = dist_A(i, j) and E = dist_B(i, j), with dist = sqrtf(d2) for mode 0 and 0.5f * d2
 * for mode 1 (the cosine / correlation distance of unit rows), d2 the float32 squared distance of mde_knn.
 * mde_pair_moments: row_sums double [n_q, 5] = the sums over j of D, E, D^2, E^2, D E (accumulated in double, the
 * products formed in double from the float32 D and E); row_max float [n_q, 2] = the row's largest D and E;
 * totals double [8] = the five sums over all rows, the largest D, the largest E, the pair count n_q (n - 1).
 * No floating-point atomics and a fixed order: for a given slice count the result is the same bits on every run,
 * and a row's sums do not depend on which other queries are listed.  Different slice counts differ by rounding.
 * mde_pair_histogram: every pair with a_lo <= D <= a_hi and b_lo <= E <= b_hi adds one to counts[bd][be],
 * bd = min(bins - 1, (int)((D - a_lo) * s_a)) with s_a = (float)bins / (a_hi - a_lo), be likewise; counts int64
 * [bins, bins] on the device is added to, so the caller zeroes it.  1 <= bins <= 64.  Integer atomics only: the
 * counts are the same for every slice count and on every run.
 * Both walk the grid of mde_knn_ranks (query block, corpus slice; slices as there, 0: automatic) with two Gram
 * tiles per step.  work: mde_pair_moments_work_bytes(n, n_q, slices) bytes of scratch for either call (the row
 * norms, the per-slice sums); the calls allocate nothing.  2 <= n < 2^31, 1 <= n_q < 2^31.  Arguments are checked
 * on the host before any launch: MDE_E_INVALID with a message.  ASYNC. */
int64_t mde_pair_moments_work_bytes(int64_t n, int64_t n_q, int32_t slices);
int mde_pair_moments(int64_t n, int32_t nfa, const float* A, int32_t mode_a, int32_t nfb, const float* B,
                     int32_t mode_b, int64_t n_q, const int32_t* q_rows, int32_t slices, double* row_sums,
                     float* row_max, double* totals, void* work, void* stream);
int mde_pair_histogram(int64_t n, int32_t nfa, const float* A, int32_t mode_a, int32_t nfb, const float* B,
                       int32_t mode_b, int64_t n_q, const int32_t* q_rows, int32_t slices, int32_t bins, float a_lo,
                       float a_hi, float b_lo, float b_hi, int64_t* counts, void* work, void* stream);
/* An embedding scored against a matrix of dissimilarities (csrc/mde_matrix_quality.hip): what the
 * matrix_* and graph_* functions of pymde_amd.quality are computed from, where D is read, not formed from data rows.
 * Dm [n, m] (float32, row-major, on the device; element offsets are 64-bit, n m may exceed 2^31) is the layout that
 * mde_graph_distances_from writes: row i is item i, column b holds the dissimilarity to item items[b].  items int32
 * [m] on the device may repeat and come in any order (an entry outside [0, n) is the caller's error and is not
 * checked); NULL: items[b] = b, and m == n.  X [n, d] (float32, row-major; 1 <= d <= 8) is the embedding.
 * A pair (i, b) does not count when items[b] == i (the item itself) or when Dm[i][b] is not finite or equals FLT_MAX
 * (a missing pair, the convention of mde_pair_loss; a NaN is skipped the same way and is the caller's error).  For a
 * counted pair D = Dm[i][b] and E = |x_i - x_items[b]|, sqrtf of the fmaf chain over the d differences as in
 * mde_pair_loss.
 * mde_matrix_moments: row_sums double [n, 5] = the sums over the row's counted pairs of D, E, D^2, E^2, D E
 * (accumulated in double, the products formed in double from the float32 D and E); row_count int64 [n] = the number
 * of counted pairs of the row; row_max float [n, 2] = the row's largest D and E (0 without a counted pair); totals
 * double [8] = the five sums over all rows, the largest D, the largest E, the total count: the layout of
 * mde_pair_moments.  No floating-point atomics and a fixed order: the same bits on every run; a row's sums depend
 * on n, m and the inputs only, never on the grid; totals come from two further launches that add the rows in
 * blocks of 4096 rows, then the blocks, both in index order.
 * mde_matrix_histogram: the same walk and the same rule; every counted pair with d_lo <= D <= d_hi and e_lo <= E <=
 * e_hi adds one to counts[bd][be], binned as in mde_pair_histogram (the last bin closed); counts int64 [bins, bins]
 * on the device is added to, so the caller zeroes it.  1 <= bins <= 64.  Integer atomics only.
 * work: mde_matrix_moments_work_bytes(n, m) bytes of scratch for mde_matrix_moments (the partial totals); the
 * histogram needs none; the calls allocate nothing.  1 <= n < 2^31, 1 <= m < 2^31.  Arguments are checked on the host
 * before any launch: MDE_E_INVALID with a message.  ASYNC. */
int64_t mde_matrix_moments_work_bytes(int64_t n, int64_t m);
int mde_matrix_moments(int64_t n, int64_t m, const float* Dm, const int32_t* items, int32_t d, const float* X,
                       double* row_sums, int64_t* row_count, float* row_max, double* totals, void* work,
                       void* stream);
int mde_matrix_histogram(int64_t n, int64_t m, const float* Dm, const int32_t* items, int32_t d, const float* X,
                         int32_t bins, float d_lo, float d_hi, float e_lo, float e_hi, int64_t* counts, void* stream);
/* Ranks within the columns of Dm (same layout): idx int32 [m, k] (1 <= k <= 64) lists items for every column, and
 * ranks[b][c] (int32 [m, k]) = the number of items j != items[b] with (Dm[j][b], j) < (Dm[l][b], l), l = idx[b][c],
 * in lexicographic order: 0-based, ties to the smaller index, the rule of mde_knn_ranks.  +inf is an ordinary value
 * that sorts last (unreachable items rank after all reachable ones, by index); a NaN is the caller's error.  An
 * entry that is negative, >= n or the column's own item gets -1 (the entries live on the device; no row is read for
 * them).  Two launches; integer arithmetic and integer atomics only: the ranks are the same for every grid and on
 * every run.  No scratch, no allocation.  Arguments are checked on the host before any launch.  ASYNC. */
int mde_matrix_ranks(int64_t n, int64_t m, const float* Dm, const int32_t* items, int32_t k, const int32_t* idx,
                     int32_t* ranks, void* stream);
/* The loss and gradient of a dense MDE problem (csrc/mde_pair_loss.hip): a loss over all
 * P = n (n - 1) / 2 pairs of n items without an edge list, what pymde_amd.DenseMDE minimises.
 * X [n, d] (float32, row-major, on the device; 1 <= d <= 8) is the embedding.  The original deviation D(i, j) of a
 * pair comes from exactly one of two sources (the other pointer is NULL):
 *   A [n, nf]   the prepared data rows: D = d_scale * dist_A(i, j), dist_A as in mde_pair_moments (mode 0 sqrtf(d2),
 *               mode 1 0.5f * d2), bit for bit the distances of that call;
 *   Dm [n, n]   a row-major float32 matrix of deviations: D = d_scale * Dm[i][j] (nf and mode are ignored).  Dm is
 *               expected to be symmetric, non-negative and finite; it is not checked, an entry equal to FLT_MAX is
 *               skipped, and the diagonal is never used.
 * For every row i and every j != i (by index): E = |x_i - x_j| from the differences, and (l, l'(E) / E) of the loss
 * `kind` (one of MDE_F_L_*; scalars s0, s1, s2 as in struct mde_func) at a0 = D and, for the weighted kinds,
 * a1 = 1 / D^2 (the losses' default weights), with the NaN / Inf -> 1 rule of mde_average_distortion on l'(E) / E.
 *   row_loss double [n]   = sum_j l(E_ij, D_ij)
 *   grad float [n, d]     = (1 / P) sum_j (l'(E_ij) / E_ij) (x_i - x_j)
 *   loss double [1]       = sum_i row_loss[i] / (2 P)
 * which are the average distortion of the edge-list problem over all_edges(n), its gradient, and the sum of the
 * distortions of the pairs of every item.  Sums in double; no floating-point atomics and a fixed order: for a given
 * slice count the three outputs are the same bits on every run; different slice counts differ by rounding.
 * The grid is that of mde_pair_moments (row block, column slice; slices as there, 0: automatic).
 * work: mde_pair_loss_work_bytes(n, d, slices) bytes of scratch (the per-slice partials, the row norms of A); the
 * call allocates nothing.  2 <= n < 2^31; d_scale positive and finite.  Arguments are checked on the host before
 * any launch: MDE_E_INVALID with a message.  ASYNC. */
int64_t mde_pair_loss_work_bytes(int64_t n, int32_t d, int32_t slices);
int mde_pair_loss(int64_t n, int32_t nf, const float* A, int32_t mode, const float* Dm, float d_scale, int32_t d,
                  const float* X, int32_t kind, float s0, float s1, float s2, int32_t slices, double* loss,
                  float* grad, double* row_loss, void* work, void* stream);
/* The rectangular form of mde_pair_loss, what pymde_amd.DensePlacement minimises: the loss of
 * every (query row i, corpus row j) pair, P = n_q n_c of them, with the corpus rows held fixed.
 * XQ [n_q, d] are the free rows and XC [n_c, d] the fixed rows of the embedding (1 <= d <= 8).  D(i, j) comes from
 * exactly one of two sources:
 *   Q [n_q, nf] and C [n_c, nf]   the prepared data rows, both given: D = d_scale * dist(q_i, c_j) through the Gram
 *               tile of Q against C (mode as in mde_pair_loss), the squared distance mde_knn_cross reports;
 *   Dm [n_q, n_c]   a row-major float32 matrix of deviations with row stride n_c, Q and C NULL: nf and mode are
 *               ignored, an entry equal to FLT_MAX is skipped, nothing else is checked.
 * Nothing is "self": a query identical to a corpus row in both spaces is an ordinary pair with D = E = 0, which adds
 * l(0, 0) to the loss and nothing to the gradient.  With E, l and l'(E) / E exactly as in mde_pair_loss:
 *   row_loss double [n_q]  = sum_j l(E_ij, D_ij)
 *   grad float [n_q, d]    = (1 / P) sum_j (l'(E_ij) / E_ij) (xq_i - xc_j)     (no gradient is formed for XC)
 *   loss double [1]        = sum_i row_loss[i] / P                             (every pair is in one row)
 * the average distortion of the edge-list problem over the bipartite pairs and the rows of its gradient that belong
 * to the query rows.  The grid is (ceil(n_q / 64), slices), slices as in mde_knn_cross (0: automatic).  Sums in
 * double, a fixed order, no floating-point atomics: for a given slice count the outputs are the same bits on every
 * run.  With Q = C and XQ = XC the row losses are those of mde_pair_loss plus the diagonal's l(0, 0).
 * work: mde_pair_loss_cross_work_bytes(n_q, n_c, d, slices) = s n_q (1 + d) 8 + 4 (n_q + n_c) bytes (the per-slice
 * partials, the row norms of Q and of C); the call allocates nothing.  1 <= n_q, n_c < 2^31.  Arguments are checked
 * on the host before any launch: MDE_E_INVALID with a message.  ASYNC. */
int64_t mde_pair_loss_cross_work_bytes(int64_t n_q, int64_t n_c, int32_t d, int32_t slices);
int mde_pair_loss_cross(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t mode,
                        const float* Dm, float d_scale, int32_t d, const float* XQ, const float* XC, int32_t kind,
                        float s0, float s1, float s2, int32_t slices, double* loss, float* grad, double* row_loss,
                        void* work, void* stream);
/* mde_pair_loss_cross over a LIST of query rows, what the per-row placement solver evaluates.
 * The arguments of mde_pair_loss_cross, then rows [n_rows] (int32, on the device): distinct query rows in any order;
 * NULL means all of them in order and requires n_rows == n_q.  1 <= n_rows <= n_q; the entries are not checked.
 * Workgroup x owns the list entries 64 x ... 64 x + 63 and reads Q, the row norms, XQ and the Dm row through the
 * list.  For every listed row i, written at the row's own index (the rows not listed are not written):
 *   row_loss double [n_q]     = sum_j l(E_ij, D_ij)
 *   row_grad float [n_q, d]   = (1 / n_c) sum_j (l'(E_ij) / E_ij) (xq_i - xc_j), rounded once from double
 * the gradient of the row's own mean loss row_loss[i] / n_c: it is divided by n_c, not by n_q n_c, so a row's result
 * does not depend on the list.  There is no loss total.  The same column order and the same fixed-order double sums
 * as mde_pair_loss_cross: at the same slice count row_loss holds the bits of that call.  slices == 0 resolves the
 * automatic count from the list's length (a short list still fills the device), so there the bits depend on n_rows.
 * work: mde_pair_loss_cross_rows_work_bytes(n_q, n_c, d, slices) bytes, enough for every list length.  ASYNC. */
int64_t mde_pair_loss_cross_rows_work_bytes(int64_t n_q, int64_t n_c, int32_t d, int32_t slices);
int mde_pair_loss_cross_rows(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t mode,
                             const float* Dm, float d_scale, int32_t d, const float* XQ, const float* XC,
                             int32_t kind, float s0, float s1, float s2, int32_t slices, int64_t n_rows,
                             const int32_t* rows, double* row_loss, float* row_grad, void* work, void* stream);
/* Per-pair weights and missing pairs for the three calls above.  Each *_weighted call takes the
 * arguments of its namesake, then the weight source `wsource`, `p`, `W` and (not the list call) `pairs`:
 *   MDE_PAIR_W_NONE     no weights: the namesake's arithmetic, with `pairs` as the divisor.  W NULL.
 *   MDE_PAIR_W_POWER    w = D^-p from the pair's own D = d_scale * deviation, formed in the kernel: no per-pair array,
 *                       either source of D.  p = 2 is 1.0f / (D * D), the bits of the losses' default weights; p = 1
 *                       is one IEEE division; p = 0 is exactly 1; any other finite p >= 0 is powf(D, -p).  D = 0 is not
 *                       special: it gives what these expressions give.  W NULL.
 *   MDE_PAIR_W_MATRIX   w = W[i][j], a row-major float32 matrix on the device, [n, n] for mde_pair_loss_weighted (both
 *                       triangles are read; it is expected to be symmetric; the diagonal is never used) and [n_q, n_c]
 *                       for the rectangular calls, with either source of D.  Only w > 0 counts: w == 0 is a MISSING
 *                       pair, skipped before anything of it is evaluated, so its Dm entry may be NaN or infinite.
 *                       p is ignored (but checked).
 * For MDE_F_L_WEIGHTED_QUADRATIC and MDE_F_L_WEIGHTED_POWER w takes the place of a1 (the reference's
 * WeightedQuadratic(deviations, weights)); for every other kind l and l'(E) / E are multiplied by w in float32, after
 * the NaN / Inf -> 1 rule.  `pairs` (double, > 0) is the number of pairs that count:
 *   mde_pair_loss_weighted         loss = sum_i row_loss[i] / (2 pairs), grad = G / pairs
 *   mde_pair_loss_cross_weighted   loss = sum_i row_loss[i] / pairs,     grad = G / pairs
 *   mde_pair_loss_cross_rows_weighted   row_grad = G / n_c as in mde_pair_loss_cross_rows: it has no `pairs`.
 * The same grid, work buffers (the namesakes' *_work_bytes), double sums and fixed order: the same bits on every run,
 * and with MDE_PAIR_W_NONE and the namesake's pair count the namesake's bits.  MDE_E_INVALID with a message, before any
 * launch, for an unknown source, W non-null without MDE_PAIR_W_MATRIX (both sources given) or NULL with it, p
 * negative or not finite, pairs not positive and finite, and whatever the namesake refuses.  ASYNC. */
#define MDE_PAIR_W_NONE 0
#define MDE_PAIR_W_POWER 1
#define MDE_PAIR_W_MATRIX 2
int mde_pair_loss_weighted(int64_t n, int32_t nf, const float* A, int32_t mode, const float* Dm, float d_scale,
                           int32_t d, const float* X, int32_t kind, float s0, float s1, float s2, int32_t slices,
                           int32_t wsource, float p, const float* W, double pairs, double* loss, float* grad,
                           double* row_loss, void* work, void* stream);
int mde_pair_loss_cross_weighted(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t mode,
                                 const float* Dm, float d_scale, int32_t d, const float* XQ, const float* XC,
                                 int32_t kind, float s0, float s1, float s2, int32_t slices, int32_t wsource, float p,
                                 const float* W, double pairs, double* loss, float* grad, double* row_loss, void* work,
                                 void* stream);
int mde_pair_loss_cross_rows_weighted(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C,
                                      int32_t mode, const float* Dm, float d_scale, int32_t d, const float* XQ,
                                      const float* XC, int32_t kind, float s0, float s1, float s2, int32_t slices,
                                      int64_t n_rows, const int32_t* rows, int32_t wsource, float p, const float* W,
                                      double* row_loss, float* row_grad, void* work, void* stream);
/* The product of the (never stored) matrix of SQUARED deviations with a thin block of vectors (csrc/mde_pair_apply.hip,
 * DESIGN section 6p): the primitive of classical scaling and of distance-based triangulation (pymde_amd.classical).
 *   out[i][k] = sum_j S(i, j) V[j][k]      i < n_q, j < n_c, k < r, 1 <= r <= 32
 * V float32 [n_c, r] (finite), out DOUBLE [n_q, r], both row-major on the device.  S(i, j) comes from exactly one of the
 * two sources of mde_pair_loss_cross:
 *   Q [n_q, nf] and C [n_c, nf]   the prepared data rows, both given; with d2 = fmaxf(|x|^2 + |y|^2 - 2 x.y, 0) the Gram
 *               tile's own squared distance (bit for bit that of mde_pair_moments): mode 0  S = d2 as it is, never
 *               sqrtf and squared again; mode 1  S = (0.5f d2)^2, the product formed in double;
 *   Dm [n_q, n_c]   a row-major float32 matrix of deviations, Q and C NULL: S = Dm[i][j]^2 formed in double, so the
 *               square is exact (nf and mode are ignored; an entry equal to FLT_MAX is skipped).
 * There is no d_scale: the product is linear, the caller scales by its square.  skip_diagonal != 0 requires n_q == n_c
 * and leaves out j == i by index: a duplicate row elsewhere is an ordinary pair, and neither a non-zero Dm[i][i] nor the
 * rounding noise of d2(i, i) counts.  The grid is (ceil(n_q / 64), slices), slices as in mde_pair_loss_cross (0:
 * automatic).  Sums in double, one fma per (pair, k), in a fixed order and without floating-point atomics: the four
 * threads of a tile row are combined in thread order and the slices are added in slice order, so for a given slice
 * count `out` is the same bits on every run and a row's result does not depend on which rows share its block.
 * work: mde_pair_sqdist_apply_work_bytes(n_q, n_c, r, slices) = (s > 1 ? s n_q r 8 : 0) + 4 (n_q + n_c) bytes (the
 * per-slice partials, the row norms of Q and of C); the call allocates nothing.  Arguments are checked on the host
 * before any launch, MDE_E_INVALID with a message: r outside [1, 32], both sources or neither, a mode other than 0 / 1,
 * skip_diagonal with n_q != n_c, sizes outside [1, 2^31), a NULL V / out / work.  ASYNC. */
int64_t mde_pair_sqdist_apply_work_bytes(int64_t n_q, int64_t n_c, int32_t r, int32_t slices);
int mde_pair_sqdist_apply(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t mode,
                          const float* Dm, int32_t skip_diagonal, int32_t r, const float* V, int32_t slices,
                          double* out, void* work, void* stream);
/* One pass over a weight matrix W [n_q, n_c] (square != 0: n_q == n_c, the diagonal is ignored) and, when Dm is not
 * NULL, over the deviations it weighs.  A pair is KEPT when its w > 0.
 *   counts int64 [5]   0 entries of W that are NaN or infinite | 1 entries that are negative | 2 kept pairs (square: of
 *                      the strict upper triangle; rectangular: all) | 3 rows without a kept pair | 4 kept entries whose
 *                      Dm is NaN, infinite or negative (square: of both triangles, as the walk reads both)
 *   tops float [4]     square only (0 otherwise): 0 max |W - W^T| | 1 max |W|, both over the finite off-diagonal
 *                      entries | 2 max |Dm - Dm^T| | 3 max Dm, both over the kept entries with a valid Dm
 *   row_kept int32 [n_q]   the kept pairs of every row (square: over j != i)
 * Integer counters only; the results do not depend on the order of the work.  The call clears its outputs.  ASYNC. */
int mde_pair_weights_check(int64_t n_q, int64_t n_c, int32_t square, const float* W, const float* Dm, int64_t* counts,
                           float* tops, int32_t* row_kept, void* stream);
/* The per-row solver of a separable problem (csrc/mde_rows.hip): n independent d-dimensional
 * minimisations (1 <= d <= 8) advanced in lock step, one BFGS iteration with a backtracking line search per row and
 * call.  State, all on the device: x [n, d], g [n, d], p [n, d], t [n] float; H [n, d, d] float (the inverse-Hessian
 * estimate); f [n] double; flags [n] int32 (bits 0-1 the status below, bit 2 "fresh": H is the identity it was reset
 * to, bits 3.. the accepted steps in a row that lowered f by at most 1e-7 |f|).  The objective of row i is
 * f_i = row_loss[i] / n_c with gradient row_grad[i, :], as mde_pair_loss_cross_rows writes them.
 *   mde_rows_init   from the evaluation at x: H = I, p = -g, t = min(1, 1 / |g|_1), fresh; a row with |g|_2 <= eps
 *                   is converged (one whose f or g is not finite is stalled).
 *   mde_rows_step   from the evaluation at x_trial, for every active row: accept when f_t and g_t are finite and
 *                   f_t <= f + 1e-4 t g.p -- BFGS update with (s, y) when s.y > 1e-10 |s| |y| (a fresh H is first
 *                   scaled to (s.y / y.y) I), adopt x, f, g; converged when |g|_2 <= eps; stalled when x_trial == x
 *                   or after two small decreases in a row; otherwise p = -H g (reset to H = I, p = -g when g.p >= 0)
 *                   and t = 1 -- else reject: t <- clamp(-g.p t^2 / (2 (f_t - f - g.p t)), 0.1 t, 0.5 t) (0.5 t when
 *                   the denominator is not positive and finite); stalled when t max|p| <= 1e-10 max(1, max|x|).
 * Both then write x_trial = x + t p for the active rows and x_trial = x for all others, whose state is not touched,
 * and counts int64 [3] = the number of rows in each status.  Float32 state; the inner products, the Armijo test and
 * the update are formed in double.  Integer atomics on counts only: the same bits on every run.  ASYNC. */
#define MDE_ROWS_ACTIVE 0
#define MDE_ROWS_CONVERGED 1
#define MDE_ROWS_STALLED 2
int mde_rows_init(int64_t n, int32_t d, int64_t n_c, float eps, const float* x, const double* row_loss,
                  const float* row_grad, double* f, float* g, float* H, float* p, float* t, int32_t* flags,
                  float* x_trial, int64_t* counts, void* stream);
int mde_rows_step(int64_t n, int32_t d, int64_t n_c, float eps, float* x, double* f, float* g, float* H, float* p,
                  float* t, int32_t* flags, float* x_trial, const double* row_loss, const float* row_grad,
                  int64_t* counts, void* stream);
/* Metrics other than Euclidean on the original data (csrc/mde_metric.hip); definitions as in
 * scipy.spatial.distance.  The reference has no metric keyword. */
#define MDE_METRIC_EUCLIDEAN 0
#define MDE_METRIC_COSINE 1      /* 1 - u.v / (|u| |v|)                  */
#define MDE_METRIC_CORRELATION 2 /* cosine of the row-centred vectors    */
#define MDE_METRIC_MANHATTAN 3   /* sum |u - v|                          */
/* Exact k nearest neighbours under the Manhattan distance, same contract as mde_knn except that d_out
 * [n, k] holds the distances themselves (not squares): idx_out [n, k] int32 (self excluded by index; -1
 * when fewer than k other rows exist), ascending per row, ties to the smaller index; 1 <= k <= 64. */
int mde_knn_l1(int64_t n, int32_t nf, const float* data, int32_t k, int32_t* idx_out, float* d_out,
               void* stream);
/* out [n, nf] = the rows of data scaled to unit length, centred first when center != 0: the Euclidean
 * search on `out` ranks by cosine (correlation) distance, d2 = 2 (1 - cos).  deg_out: int32 [2] on the
 * device = (number of rows without a direction -- zero norm, or constant when centring --, index of the
 * first such row; INT32_MAX when there is none); those rows come out all zero, never NaN.  out may be
 * NULL (the check alone). */
int mde_rows_normalize(int64_t n, int32_t nf, const float* data, int32_t center, float* out,
                       int32_t* deg_out, void* stream);
/* out[e] = distance under `metric` (MDE_METRIC_COSINE, _CORRELATION or _MANHATTAN) between rows i and j of data [n, nf] for every edge
 * (i, j) of edges [p, 2] (int64): one pass over the two rows, sums in double, no normalised copy, so
 * near-duplicate rows keep their small distances.  NaN for an endpoint outside [0, n) and where the
 * distance is undefined (a zero row under cosine, a constant row under correlation). */
int mde_pair_distances_metric(int64_t n, int32_t nf, const float* data, int64_t p, const int64_t* edges,
                              int32_t metric, float* out, void* stream);
/* Bit-packed binary data (csrc/mde_bits.hip).  A matrix of n rows and nf 0/1 features,
 * 1 <= nf < 2^24, is words int32 [n, nw], nw = ceil(nf / 32), row-major on the device: feature f is bit f & 31 of
 * word f >> 5 and every padding bit is zero; counts int32 [n] are the row popcounts.  With a, b the counts of two
 * rows and t the popcount of the AND of their words, a pair's distance is one correctly rounded float32 quotient
 * of exact integers, the definitions of scipy.spatial.distance:
 *   kind 0  Jaccard  (a + b - 2 t) / (a + b - t), 0 when a + b - t == 0 (two empty rows)
 *   kind 1  Hamming  (a + b - 2 t) / nf
 * so a pair has the same bits in every function below and for every slice count.
 * mde_bits_pack: data float32 [n, nf] -> words and counts (one wave per row, a 64-lane ballot of x != 0 is two
 * words).  bad_row int32 [1] on the device = the first row that holds a value other than 0 or 1, NaN included
 * (INT32_MAX when there is none; the words of such a row mean nothing).
 * mde_bits_pack_csr: the same from CSR (indptr int64 [n + 1], indices int32 [nnz], values float32 [nnz]): the
 * stored values are what is checked, a stored 0 sets nothing, a duplicate entry sets its bit once (integer
 * atomic OR into zeroed words; the counts are taken from the words), and a column outside [0, nf) makes the row
 * bad.  Arguments are checked on the host before any launch: MDE_E_INVALID with a message.  ASYNC. */
int mde_bits_pack(int64_t n, int32_t nf, const float* data, int32_t* words, int32_t* counts, int32_t* bad_row,
                  void* stream);
int mde_bits_pack_csr(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                      const float* values, int32_t* words, int32_t* counts, int32_t* bad_row, void* stream);
/* Exact k nearest rows of C [n_c, nw] for every row of Q [n_q, nw] under `kind`, the contract of mde_knn_cross:
 * idx_out [n_q, k] int32 (-1 in the slots beyond the rows available), dist_out [n_q, k] float32 distances (not
 * squares), each row ordered by (value, index); 1 <= k <= 64; n_q, n_c < 2^31; nw == ceil(nf / 32).
 * self != 0: Q == C, q_counts == c_counts and n_q == n_c (the self-join); only the pair of a row with itself is
 * excluded, so duplicate rows list each other at 0.  slices as in mde_knn_cross (grid (query block of 64 rows,
 * corpus slice); 0: automatic; the per-slice lists are folded by (value, index)): the result is bit-identical for
 * every slice count and on every run.  No floating-point atomics.
 * work: mde_bits_knn_work_bytes(n_q, n_c, k, slices) bytes of scratch (the per-slice lists; 8 bytes with one
 * slice); the call allocates nothing.  Arguments are checked on the host before any launch: MDE_E_INVALID with
 * a message.  ASYNC. */
int64_t mde_bits_knn_work_bytes(int64_t n_q, int64_t n_c, int32_t k, int32_t slices);
int mde_bits_knn(int64_t n_q, int64_t n_c, int32_t nw, int32_t nf, const int32_t* Q, const int32_t* q_counts,
                 const int32_t* C, const int32_t* c_counts, int32_t self, int32_t kind, int32_t k, int32_t slices,
                 int32_t* idx_out, float* dist_out, void* work, void* stream);
/* out[e] = the distance under `kind` between rows i and j of the packed matrix for every edge (i, j) of edges
 * [p, 2] (int64), with the bits mde_bits_knn gives the pair.  NaN for an endpoint outside [0, n). */
int mde_bits_pair_distances(int64_t n, int32_t nw, int32_t nf, const int32_t* words, const int32_t* counts, int64_t p,
                            const int64_t* edges, int32_t kind, float* out, void* stream);
/* Approximate k-NN by an inverted file (csrc/mde_ann.hip) [ref: preprocess/data_matrix.py:125-143].
 * Query-against-base search restricted to block-sparse (query tile, candidate range) pairs.  Query
 * position p reads row q_map[p] of Q [n_q, nf] (q_map NULL: row p), base position c reads row b_map[c] of
 * B [n_b, nf]; q_sqn / b_sqn are the row norms (mde_row_sqnorm).  List l is the base positions
 * [offsets[l], offsets[l + 1]) (offsets int64 [n_lists + 1], non-decreasing, offsets[n_lists] <= n_bpos).
 * tiles int64 [n_tiles, 3] = (q_lo, q_hi, l): query positions [q_lo, q_hi), 1 to 64 of them, are searched
 * against the lists probe[l * n_probe + 0 .. n_probe - 1] (probe int32 [n_lists, n_probe], ids < n_lists).
 * flags: 1 = skip a candidate whose B row equals the query's Q row (Q and B the same matrix), 2 = write the
 * result of query position p at row q_map[p] (its row of Q, outputs [n_q, k]) instead of at row p
 * (outputs [n_qpos, k]).  idx_out int32 [., k]: B rows (the original index), -1 where fewer than k
 * candidates exist; d2_out [., k] squared distances; each row ordered by (d2, index), so the result does
 * not depend on the probe order and is the same on every run.  1 <= k <= 64; n_q, n_b < 2^31.  Offsets,
 * probe ids, tiles and row maps are checked on the host first: MDE_E_INVALID before any launch.  SYNC
 * (the check; the search itself is enqueued). */
int mde_ann_search(int32_t nf, int32_t k, int32_t flags, int64_t n_q, const float* Q, const float* q_sqn,
                   int64_t n_qpos, const int32_t* q_map, int64_t n_b, const float* B, const float* b_sqn,
                   int64_t n_bpos, const int32_t* b_map, int64_t n_lists, const int64_t* offsets,
                   int32_t n_probe, const int32_t* probe, int64_t n_tiles, const int64_t* tiles,
                   int32_t* idx_out, float* d2_out, void* stream);
/* centroids[l] = mean of the rows members[offsets[l] .. offsets[l + 1] - 1] of data [n, nf], summed in
 * membership order in double (one workgroup per list, no atomics: bit-reproducible); an empty list keeps
 * the centroid it had.  members int32 [n_members] (< n), offsets as for mde_ann_search (<= n_members),
 * centroids [n_lists, nf].  Checked on the host first (MDE_E_INVALID before any launch).  SYNC (the check). */
int mde_ann_centroids(int64_t n, int32_t nf, const float* data, int64_t n_members, const int32_t* members,
                      int64_t n_lists, const int64_t* offsets, float* centroids, void* stream);
/* One neighbour-of-neighbour pass over k-NN lists (csrc/mde_ann_refine.hip).  X [n, nf] are
 * the prepared float32 rows and sqn their norms (mde_row_sqnorm).  idx_in int32 [n, k] / d2_in [n, k]: each
 * row's valid entries ascending by (d2, index), -1 slots trailing, no self entry, no row twice.  rev int32
 * [n, k]: reverse neighbours of every row (rows that list it), -1 padded.  Row i's candidates are rev[i] and
 * the lists of every row of idx_in[i] and rev[i]; idx_out / d2_out (not the inputs: the pass reads the previous
 * lists throughout) receive the k smallest of the old entries and the candidates under (d2, index), in the
 * form of the inputs, empty slots as (-1, FLT_MAX).  A candidate's d2 is the float32 value the Euclidean
 * searches give the pair, bit for bit, so an exact list is a fixed point.  changed_out: int32 on the device,
 * the number of rows whose list changed.  work: mde_knn_refine_work_bytes(n, k) bytes; afterwards its first
 * uint64 holds the number of distances the pass evaluated.  The output is the same on every run.
 * 1 <= k <= 64, 1 <= n < 2^31; MDE_E_INVALID otherwise (the byte count: a negative MDE_E_* code). */
int64_t mde_knn_refine_work_bytes(int64_t n, int32_t k);
int mde_knn_refine(int64_t n, int32_t nf, const float* X, const float* sqn, int32_t k, const int32_t* idx_in,
                   const float* d2_in, const int32_t* rev, int32_t* idx_out, float* d2_out, int32_t* changed_out,
                   void* work, void* stream);
/* Landmark selection (csrc/mde_landmarks.hip): m distinct rows of data [n, nf], chosen one after
 * the other from every row's squared distance to its nearest landmark so far.  method 0: farthest point (the row
 * with the largest such distance, ties to the smallest row); method 1: k-means++ (the smallest row whose inclusive
 * prefix sum of those distances, float64 in row order, exceeds u_t * total, u_t the top 53 bits of draw t of the
 * SplitMix64 stream of seed; the smallest unselected row when the total is 0).  Position 0 is `start`.  The
 * distance is the float32 sum_f (x_f - l_f)^2, exactly 0 between equal rows, summed in an order fixed by nf.
 * idx_out int32 [m]: the rows in selection order; radius2_out [m]: each one's squared distance to the landmarks
 * before it (+inf at position 0); mind2_out [n]: every row's squared distance to its nearest landmark (0 for the
 * landmarks); nearest_out int32 [n]: the position in idx_out of that landmark, ties to the earlier one.  mind2_out
 * and nearest_out are also the state of the run.  work: mde_select_landmarks_work_bytes(n, nf, m) bytes.  All of it
 * is enqueued on the stream (2 m + 1 launches, nothing is read back); the same bits on every run and for every grid.
 * 1 <= m <= n < 2^31, 1 <= nf <= 2^30, 0 <= start < n: MDE_E_INVALID / MDE_E_TOO_LARGE otherwise (the byte count: a
 * negative MDE_E_* code). */
int64_t mde_select_landmarks_work_bytes(int64_t n, int32_t nf, int64_t m);
int mde_select_landmarks(int64_t n, int32_t nf, const float* data, int64_t m, int32_t method, int64_t start,
                         uint64_t seed, int32_t* idx_out, float* radius2_out, float* mind2_out,
                         int32_t* nearest_out, void* work, void* stream);
/* Sparse data matrices (SURVEY 8f rows f2 / f4 on scipy.sparse inputs) [ref: preprocess/data_matrix.py:11-178].
 * Every entry below takes one device CSR of n rows and nf columns: indptr int64 [n + 1], indices int32
 * [nnz] (column ids, strictly increasing within a row), values float32 [nnz]; n < 2^31, nf < 2^31, nnz may
 * exceed 2^31, rows may be empty.  Each validates the CSR on the device first (reads stay inside the
 * arrays) and returns MDE_E_INVALID with a message when indptr[0] != 0, indptr decreases, indptr[n] != nnz,
 * a column id lies outside [0, nf) or a row's ids are not strictly increasing.  SYNC (the validation). */
int mde_sparse_validate(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                        const float* values, void* stream);
/* Exact k nearest neighbours (Euclidean) of every row of the CSR, same contract as mde_knn: idx_out [n, k]
 * int32 (self excluded by index; -1 when fewer than k other rows exist), d2_out [n, k] squared distances
 * ascending per row, ties to the smaller index; 1 <= k <= 64; sqn_work: n floats of scratch (row squared
 * norms).  Bit-reproducible from run to run.  SYNC (the validation; the search itself is enqueued). */
int mde_sparse_knn(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                   const float* values, int32_t k, int32_t* idx_out, float* d2_out, float* sqn_work,
                   void* stream);
/* The number of feature columns per window of mde_sparse_knn(k) on a matrix of nf columns: the search walks
 * a row's stored entries one window at a time, 64 entries per step, so a row with 64 or more entries inside
 * one window takes more than one step there.  A multiple of 8.  Host only, nothing is launched.  k outside
 * [1, 64] or nf < 1: MDE_E_INVALID with a message. */
int32_t mde_sparse_knn_window(int32_t k, int32_t nf);
/* out[e] = ||x_i - x_j|| for every edge (i, j) of edges [p, 2] (int64), summed over the union of the two
 * rows' columns as (a - b)^2 in double -- no cancellation, near-duplicate rows come out near zero.  An
 * endpoint outside [0, n) gives NaN.  Reproducible from run to run.  SYNC (the validation). */
int mde_sparse_distances(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                         const float* values, int64_t p, const int64_t* edges, float* out, void* stream);
/* values_out[e] = values[e] / |row of e|: the CSR with unit rows (same indptr / indices), on which
 * mde_sparse_knn / mde_sparse_distances rank by cosine, d2 = 2 (1 - cos).  deg_out: int32 [2] on the device
 * = (number of rows with zero norm, index of the first; INT32_MAX when none).  SYNC (the validation). */
int mde_sparse_rows_normalize(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr,
                              const int32_t* indices, const float* values, float* values_out,
                              int32_t* deg_out, void* stream);
/* C = A B - u v^T for the CSR A [n, nf] and a dense row-major B [nf, r] float32, 1 <= r <= 256:
 *   C[i, c] = sum over the stored entries e of row i of values[e] * B[indices[e], c]  -  u[i] * v[c],
 * C [n, r] float32; u float32 [n] or NULL (all ones); v DOUBLE [r] or NULL (no correction).  The rank-one term
 * centres a sparse matrix without densifying it: (A - 1 mu^T) B = A B - 1 (mu^T B); on the transposed CSR,
 * (A - 1 mu^T)^T Q = A^T Q - mu (1^T Q).  Products and sums in float64, a row's entries in ascending column
 * order, the correction subtracted in float64, one rounding to float32 at the store.  A row longer than
 * mde_csr_spmm_segment() entries is cut into segments of that many entries, summed by different waves into
 * float64 partials in `work` and added in segment order by a second launch; no atomics, the same bits on every
 * run.  work: mde_csr_spmm_work_bytes(n, nnz, r) bytes (a bound that does not read the row pointers: two float64
 * [r] slots per segment length of nnz; a negative MDE_E_* code for invalid sizes), need not be initialised.
 * UNLIKE the entries above this one does NOT validate the CSR: the precondition is a canonical CSR that
 * mde_sparse_validate accepts (the caller validates once per matrix, not once per product).  r outside
 * [1, 256], negative sizes and NULL pointers: MDE_E_INVALID with a message, nothing launched.  ASYNC. */
int32_t mde_csr_spmm_segment(void);
int64_t mde_csr_spmm_work_bytes(int64_t n, int64_t nnz, int32_t r);
int mde_csr_spmm(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                 const float* values, int32_t r, const float* B, const float* u, const double* v, float* C,
                 void* work, void* stream);
/* Shortest-path distances on the graph whose edges built `plan` (a FULL plan; its symmetrised CSR
 * is the adjacency) [ref: preprocess/graph.py:286-474, _graph.pyx:10-52].
 * w: per-half-edge edge lengths in plan (CSR) order (mde_plan_expand), or NULL for unit lengths
 * (BFS).  For every pair i < j at finite positive distance <= max_length (<= 0: no limit) the pair is
 * kept with probability retain_fraction (>= 1: all), decided by a hash of (seed, i, j).  Writes the
 * kept pairs sorted by (i, j) to edges_out [capacity, 2] / dist_out [capacity]; *count_host = their
 * number (fails with MDE_E_INVALID, count still reported, when it exceeds `capacity`).  SYNC. */
int mde_graph_shortest_paths(const mde_plan* plan, const float* w, float max_length,
                             double retain_fraction, uint64_t seed, int64_t capacity,
                             int64_t* edges_out, float* dist_out, int64_t* count_host, void* stream);
/* Edge list of directed neighbour lists: pairs_out[r * k + c] = (r, idx[r][c]); empty slots (idx < 0)
 * and entries with val > max_value (val may be NULL) become self pairs, which
 * mde_edges_count_unique drops [ref: preprocess/data_matrix.py:147-175]. */
int mde_knn_pairs(int64_t n, int32_t k, const int32_t* idx, const float* val, float max_value,
                  int64_t* pairs_out, void* stream);
/* Per-row calibration of edge affinities over directed neighbour lists.  idx [n, k] int32
 * (-1 = empty slot), val [n, k] float32, 1 <= k <= 64, n k < 2^31 - 1.  An entry is MISSING when its idx is
 * outside [0, n) or equals its row, or when has_max != 0 and !(val <= max_value) (the rule of mde_knn_pairs);
 * the others are the row's k_i kept entries, at distance d = scale * (root ? sqrt(max(val, 0)) : val) formed in
 * double (scale > 0).
 *   kind 0, perplexity > 0: s_j = d_j^2 - min_j d_j^2, p_j = exp(-beta s_j) / sum, beta >= 0 the root of
 *     -sum p log p = log(perplexity).  c = #{s_j = 0}.  perplexity >= k_i or c == k_i: p = 1 / k_i, beta = 0;
 *     perplexity <= c: 1 / c on the entries with s_j = 0 and 0 elsewhere, beta = +inf.  bandwidth = beta,
 *     offset = min_j d_j.
 *   kind 1 (UMAP's smooth k-NN distances; perplexity is not read): rho = the smallest positive d_j (0 when
 *     there is none), g_j = max(d_j - rho, 0), p_j = exp(-g_j / sigma), sigma the root of sum_j p_j = log2(k_i),
 *     then raised to at least 1e-3 * mean_j d_j.  c = #{g_j = 0}.  c == k_i: all ones (sigma = that floor);
 *     log2(k_i) <= c: the root is the limit sigma -> 0, so sigma = the floor and p_j = exp(-g_j / floor).
 *     bandwidth = sigma, offset = rho.
 * Roots by bisection in double until the bracket is below 2^-48 of its upper end (at most 400 steps); sums in a
 * fixed order; one rounding to float32 per output.  idx_out [n, k] = idx with -1 at every missing entry, p_out
 * [n, k] (0 at missing entries), bandwidth_out [n], offset_out [n]; a row with k_i = 0 writes zeros.  The same
 * bits on every run.  ASYNC. */
int mde_knn_calibrate(int64_t n, int32_t k, const int32_t* idx, const float* val, int32_t root, double scale,
                      int32_t has_max, float max_value, int32_t kind, double perplexity, int32_t* idx_out,
                      float* p_out, float* bandwidth_out, float* offset_out, void* stream);
/* Undirected edges of directed neighbour lists with combined weights.  idx [n, k] (the idx_out above: -1 =
 * no entry; the kept entries of a row distinct and none of them the row itself), p [n, k] float32.  For the
 * edge {i, j}, i < j: a = p[i][slot of j] (0 when i does not list j), b the same from row j;
 *   rule 0 (mean): w = 0.5f * (a + b) in float32;   rule 1 (union): w = (float)(a + b - a b) in double.
 * edges_out [>= n k, 2] int64 and weights_out [>= n k] receive each edge once, i < j, sorted by (i, j): the
 * edge set and order of mde_knn_pairs + mde_edges_count_unique on the same lists (an edge whose weight is 0
 * stays).  *count_host = their number.  n k < 2^31 - 1.  SYNC. */
int mde_knn_symmetrize(int64_t n, int32_t k, const int32_t* idx, const float* p, int32_t rule,
                       int64_t* edges_out, float* weights_out, int64_t* count_host, void* stream);
/* k nearest neighbours of every vertex under the graph's shortest-path metric (direct = 0) or among
 * its graph neighbours by edge length (direct = 1) [ref: preprocess/graph.py:502-587].  plan / w /
 * max_length as for mde_graph_shortest_paths.  idx_out [n, k] int32 (-1 = fewer than k targets
 * within max_length), dist_out [n, k] ascending; ties go to the smaller index.  SYNC. */
int mde_graph_knn(const mde_plan* plan, const float* w, float max_length, int32_t direct, int32_t k,
                  int32_t* idx_out, float* dist_out, void* stream);
/* Shortest-path lengths from a list of source nodes to every node.  plan, w and max_length as
 * for mde_graph_shortest_paths; sources [m] int64 (device or host memory): node indices in any order, repeats
 * allowed.  out [n, m] float32, one row per node: out[v * m + b] is the length from sources[b] to v, 0 at the source,
 * +inf where no path exists or none of length <= max_length.  Every value is the minimum over paths of the float32
 * left-to-right sum of the edge lengths from the source, so the bits do not depend on the run or the grid and equal
 * those of mde_graph_shortest_paths for the pair.  MDE_E_INVALID (nothing launched) for a sharded plan, NULL
 * pointers, m < 1 or a source outside [0, n); MDE_E_INVALID also when n sweeps do not reach the fixed point
 * (negative lengths).  Work memory: 16 n ceil(m / 4096) + 4 n bytes.  SYNC. */
int mde_graph_distances_from(const mde_plan* plan, const float* w, float max_length, int64_t m,
                             const int64_t* sources, float* out, void* stream);
/* What the calling thread's last mde_graph_distances_from did: stats[0] sweeps, [1] tiles (a node x 64 consecutive
 * columns) relaxed over all sweeps, [2] tiles per sweep, [3] nodes handled by the many-wave kernel. */
int mde_graph_distances_stats(int64_t* stats);
/* The connected components of the graph of a full (unsharded) plan (csrc/mde_graph_components.hip, DESIGN section
 * 6u).  labels_out [n] int32 on the device: the label of a node is the rank of its component when the components are
 * ordered by their smallest node (0 for the component of node 0, and so on: the numbering of
 * scipy.sparse.csgraph.connected_components); *count_host = the number of components.  Edge values are not read: an
 * edge of length 0 or inf joins its ends like any other.  Hooking and pointer jumping on one parent array (integer
 * atomicMin; the fixed point -- every node at the smallest node of its component -- is unique, so the output is the
 * same on every run): a round is a hook launch (two when some row has more than 64 neighbours: those take a wave
 * each), a jump launch and a 4-byte read-back; the number of rounds grows with log n, not with the hop diameter.
 * MDE_E_INVALID (nothing launched) for NULL pointers or a sharded plan, and if 256 rounds do not reach the fixed
 * point.  Work memory: 12 n bytes.  SYNC. */
int mde_graph_components(const mde_plan* plan, int32_t* labels_out, int64_t* count_host, void* stream);
/* What the calling thread's last mde_graph_components did: stats[0] rounds (the last one changed nothing; 0 for a
 * graph without edges), [1] kernel launches, [2] hook operations that lowered a slot of the parent array. */
int mde_graph_components_stats(int64_t* stats);
/* Sample at most num_edges distinct edges i < j uniformly at random from the edges NOT in
 * `exclude` [n_exclude, 2] (NULL / 0: no exclusion); edges_out must hold num_edges rows, sorted by
 * (i, j); *count_host = number written (== num_edges unless the complement is nearly exhausted).
 * Same `seed` -> same edges.  Rounds of draws (draw t of a round's seed: mde_rng.h; pair index -> edge:
 * mde_tri_index.h) are de-duplicated and filtered until num_edges survive; a surplus is thinned at random, by the
 * rank splitmix64(salt(seed) ^ key); a round that would draw at least C(n, 2) times offers every pair once, so
 * a request on a small n is an exactly uniform subset and never falls short.  SYNC. */
int mde_sample_edges(int64_t n, int64_t num_edges, uint64_t seed, const int64_t* exclude,
                     int64_t n_exclude, int64_t* edges_out, int64_t* count_host, void* stream);

/* ------------------------------------------------------------------ the hot kernel
 * Fused forward + backward of the average distortion
 *   E(X) = (1/p) sum_k f_k(||x_ik - x_jk||),  dE/dX          [ref: average_distortion.py:62-106]
 * `f->a0/a1` are in PLAN (half-edge) order (mde_plan_expand) unless *_scalar is set.
 * Writes rows [row_lo,row_hi) of grad (other rows untouched) when grad != NULL, and the
 * plan's share of E into *loss_out (device float; full E for a full plan).  With
 * grad == NULL this is the forward-only evaluation (average_distortion.py:90-91).
 * g_k = f'_k(d_k)/(p d_k) with NaN -> 1, Inf -> 1 as in average_distortion.py:81-88.
 * `grad_scale` multiplies the gradient (upstream grad_output, average_distortion.py:105).
 */
int mde_average_distortion(mde_plan* plan, const float* X, int32_t d, const mde_func* f,
                           float grad_scale, float* grad, float* loss_out, void* stream);

/* ------------------------------------------------------------------ edge-order evaluators
 * [ref: problem.py:246-308 differences / distances / distortions; average_distortion.py:38-55]
 * These work on the caller's ORIGINAL edge order and need no plan. */
int mde_differences(int64_t n, int64_t p, const int64_t* edges, const float* X, int32_t d,
                    float* diff_out /* [p,d] */, void* stream);
int mde_distances(int64_t n, int64_t p, const int64_t* edges, const float* X, int32_t d,
                  float* dist_out /* [p] */, void* stream);
/* backward of distances: grad_X += sum_k gout_k (x_i - x_j)/d_k (+ to i, - to j), NaN -> 0
 * (average_distortion.py:46-52).  Needs a full plan of the same edges; gout in edge order. */
int mde_distances_backward(const mde_plan* plan, const float* X, int32_t d, const float* gout,
                           float* grad /* [n,d], rows of the plan overwritten */, void* stream);
/* out_k = f_k(dist_k) and, when dout != NULL, dout_k = f'_k(dist_k); parameters in EDGE order. */
int mde_distortions(int64_t p, const float* dist, const mde_func* f, float* out, float* dout,
                    void* stream);

/* Unfused fallback for arbitrary Python callables (average_distortion.py:73-105):
 * grad[v] = scale * sum_h gfix(gnorm[eid[h]] / dist[eid[h]]) (x_v - x_nbr), where
 * gnorm = d(mean f)/d(dist) from torch autograd and gfix maps NaN/Inf to 1.0 (:81-88). */
int mde_scatter(const mde_plan* plan, const float* X, int32_t d, const float* gnorm,
                const float* dist, float scale, float* grad, void* stream);

/* ------------------------------------------------------------------ constraints
 * [ref: constraints.py:94-200, util.py:129-171] */
/* Z -= column mean (Centered retraction, constraints.py:106-111). `work` >= mde_work_doubles(d). */
int mde_center(int64_t n, int32_t d, float* Z, double* work, void* stream);
/* Anchored (constraints.py:143-164): rows[anchors] = values (or 0 when values == NULL). */
int mde_anchor_rows(int64_t n_anchors, int32_t d, const int64_t* anchors, const float* values,
                    float* Z, void* stream);
/* Rows on a sphere (constraints.py:203-231, `_Sphere`: private in the reference, used by no recipe).
 * X == NULL: the retraction Z[r] <- (Z[r] / |Z[r]|) * radius (:225-231); else the tangent projection
 * Z[r] -= (1 / radius) (Z[r] . X[r]) X[r] (:214-223; the reference's own scale, 1 / radius). */
int mde_sphere_rows(int64_t n, int32_t d, const float* X, float* Z, float radius, void* stream);
/* Standardized tangent projection Z -= (1/n) X (Z^T X)  (constraints.py:186-192). */
int mde_std_tangent(int64_t n, int32_t d, const float* X, float* Z, double* work, void* stream);
/* Standardized retraction: Z <- sqrt(n) * polar factor of (Z - mean)  (util.py:129-161),
 * computed as sqrt(n) (Z-mean) C^{-1/2}, C = (Z-mean)^T (Z-mean), with C^{-1/2} from a closed
 * form (d <= 2) or a coupled Newton-Schulz iteration in double on the device.  status_dev (device
 * int32, may be NULL) is set non-zero when C is numerically singular.  demean = 0 skips the
 * centring (util.py:130-134).  ASYNC for d < 32; for d >= 32 the iteration's residual words are
 * read back after every batch of steps (one stream synchronisation per 6 steps, usually one). */
int mde_std_retract(int64_t n, int32_t d, float* Z, int32_t demean, double* work,
                    int32_t* status_dev, void* stream);
/* The line search's trial point in one call: Z <- retraction(X + t dir) for the Centered and the
 * Standardized constraint [ref: optim.py:135-136 after lbfgs.py:551: `X += t d` then
 * `constraint.project_onto_constraint(X)`].  At small d the step is folded into the first pass of the
 * retraction (one launch less per trial); results are those of mde_axpy followed by mde_center /
 * mde_std_retract, bit for bit. */
int mde_center_step(int64_t n, int32_t d, const float* X, const float* dir, float t, float* Z, double* work,
                    void* stream);
int mde_std_retract_step(int64_t n, int32_t d, const float* X, const float* dir, float t, float* Z,
                         int32_t demean, double* work, int32_t* status_dev, void* stream);
/* mde_center_step in two halves, for a solve whose rows are sharded across ranks: _begin forms this rank's n rows of
 * Z = X + t dir (dir == NULL: Z as it is) and leaves the column MEANS over those rows in work[0 .. d) (device doubles);
 * the caller sums them across the ranks in place (one small all-reduce); _end subtracts scale x work[0 .. d) from the
 * rows (scale = n / n_total, this rank's share of the rows).  In a world of one: _begin + _end(scale 1) = mde_center_step. */
int mde_center_step_begin(int64_t n, int32_t d, const float* X, const float* dir, float t, float* Z, double* work,
                          void* stream);
int mde_center_step_end(int64_t n, int32_t d, float* Z, double* work, double scale, void* stream);
/* mde_std_tangent(X, Z) followed by mde_vec_stats(Z, dir, X) (dir may be NULL): the projected gradient
 * and the statistics the line search reads, with the statistics folded into the projection's second
 * pass at d <= 4.  ASYNC. */
int mde_std_tangent_stats(int64_t n, int32_t d, const float* X, float* Z, const float* dir, double* stats,
                          double* work, void* stream);
/* Gram matrix out[d_a, d_b] (double, device) = A^T B for A [n,d_a], B [n,d_b]; uses the
 * f32 MFMA path when both widths are multiples of 32. */
int mde_gram(int64_t n, int32_t da, int32_t db, const float* A, const float* B, double* out,
             double* work, void* stream);
/* Z = A M, M [d, d2] device double row-major (small). */
int mde_right_multiply(int64_t n, int32_t d, int32_t d2, const float* A, const double* M,
                       float* out, void* stream);
/* out = base + alpha * A M  (base may be NULL or alias out; out may alias A only when d == d2). */
int mde_right_multiply_add(int64_t n, int32_t d, int32_t d2, const float* A, const double* M,
                           float alpha, const float* base, float* out, void* stream);
/* Z[r, :] += shift (d device doubles): the translation part of util.align [ref: util.py:302-331]. */
int mde_shift_rows(int64_t n, int32_t d, const double* shift, float* Z, void* stream);
/* Z[r, :] *= scale[r]  (row scaling, e.g. the Jacobi preconditioner of the spectral initialiser). */
int mde_row_scale(int64_t n, int32_t d, const float* scale, float* Z, void* stream);
/* out[v] = sum of the per-edge weights (plan / CSR order) over the half-edges of row v: the diagonal
 * of the graph Laplacian [ref: quadratic.py:47-68].  Rows outside the plan's range are untouched. */
int mde_weighted_degree(const mde_plan* plan, const float* w_plan_order, float* out, void* stream);
/* number of doubles of scratch the constraint / gram / vector calls need for width d.  ZERO the
 * buffer once after allocating it: a few of its words are the arrival counters of the kernels that
 * finish their reduction in the last workgroup (they are back at zero after every call).  One
 * buffer serves one stream at a time. */
int64_t mde_work_doubles(int32_t d);

/* ------------------------------------------------------------------ vector kernels
 * [ref: lbfgs.py:350-376, 461-530; optim.py:94-147]  flat float32 vectors of length N */
/* out = y + alpha x  (lbfgs.py:350-357 `_add_grad`);  out may alias y */
int mde_axpy(int64_t N, float alpha, const float* x, const float* y, float* out, void* stream);
/* stats[0..7] (device doubles) = { g.d, g.g, sum|g|, max|g|, #non-finite(g), d.d, max|d|, x.x }
 * (d and x may be NULL: their entries are 0).  One pass.  lbfgs.py:59, 82, 523, 527; optim.py:96, 130 */
int mde_vec_stats(int64_t N, const float* g, const float* d, const float* x, double* stats,
                  double* work, void* stream);

/* ------------------------------------------------------------------ L-BFGS memory
 * [ref: lbfgs.py:461-507]  Device-resident history of (s, y) pairs with one spare slot. */
typedef struct mde_lbfgs mde_lbfgs;
int mde_lbfgs_create(int64_t N, int32_t history, mde_lbfgs** out);
int mde_lbfgs_destroy(mde_lbfgs* o);
/* The whole direction update of one iteration without a host round trip [ref: lbfgs.py:468-507]: the
 * bookkeeping (slot order, Gram matrices of the stored pairs, coefficients) lives on the device.
 * mde_lbfgs_dev_reset empties the history (lbfgs.py:378-388; call it once after mde_lbfgs_create);
 * mde_lbfgs_dev_step stages y = g - g_prev, s = t d in the spare slot (and sets g_prev <- g), accepts
 * the pair iff y.s > 1e-10 (dropping the oldest when the history is full), runs the two-loop recursion
 * in coefficient form on the device and writes the new direction to d_out (may alias d) and the
 * statistics of (g, d_out) to stats as mde_vec_stats(g, d_out, NULL) does.  ASYNC.  mde_lbfgs_dev_info
 * reads back the number of stored pairs and whether the last pair was accepted (tests; SYNC). */
int mde_lbfgs_dev_reset(mde_lbfgs* o, void* stream);
int mde_lbfgs_dev_step(mde_lbfgs* o, const float* g, float* g_prev, const float* d, float t,
                       float* d_out, double* stats, double* work, void* stream);
int mde_lbfgs_dev_info(const mde_lbfgs* o, int32_t* count_host, int32_t* accepted_host, void* stream);
/* The same step in two halves, for a solve whose vectors are SHARDED BY ROWS across ranks (every rank keeps the
 * history of its own rows: mde_lbfgs_create(N = its elements)) [ref: lbfgs.py:461-507, the loop being sharded]:
 * mde_lbfgs_dev_stage stages the pair and leaves the mde_lbfgs_dev_dots(o) = 4 + 5 * history inner products over the
 * rank's elements in work[0 ..) (device doubles: [0] y.s [1] y.y [2] s.g [3] y.g, then for each stored pair j, oldest
 * first: s_j.y, y_j.y, s.y_j, s_j.g, y_j.g); the caller sums them across the ranks IN PLACE (one small
 * all-reduce); mde_lbfgs_dev_finish takes the accept / drop-oldest decision and runs the two-loop recursion on the
 * sums (every rank: the same arithmetic on the same numbers) and writes the rank's elements of the new direction to
 * d_out and the statistics of (g, d_out) over ITS elements to stats (partial: see mde_rank_reduce).  In a world of
 * one, stage + finish = mde_lbfgs_dev_step's four-launch form.  ASYNC. */
int mde_lbfgs_dev_stage(mde_lbfgs* o, const float* g, float* g_prev, const float* d, float t, double* work, void* stream);
int mde_lbfgs_dev_finish(mde_lbfgs* o, const float* g, float* d_out, double* stats, double* work, void* stream);
int32_t mde_lbfgs_dev_dots(const mde_lbfgs* o);
/* out[q] = sum -- or max, where bit q of max_mask is set -- over the ranks r (in rank order) of in[r * count + q],
 * q < count <= 64, device doubles; loss_slot >= 0: that result is also written to *loss_out as a float.  Reduces the
 * per-rank records of a sharded solve (statistics boards + loss shares, exchanged with ONE all-gather) in one launch. */
int mde_rank_reduce(int32_t world, int32_t count, uint64_t max_mask, const double* in, double* out,
                    int32_t loss_slot, float* loss_out, void* stream);
/* Which form mde_lbfgs_dev_step takes (process-wide; read from the environment on first use:
 * MDE_LB_UNFUSED, MDE_LB_DEBUG = "blocks,spins,lds_bytes").  For N <= 2^18 the step is ONE launch whose
 * workgroups meet at grid-wide arrival points; an ordinary launch cannot guarantee that they are all
 * resident, so a workgroup that waits longer than `spins` polls gives up and a rescue kernel queued
 * behind redoes the step from the staged sums -- the direction is the four-launch path's either way.
 * unfused != 0 forces the four launches; blocks / spins / lds_bytes > 0 (tests) launch that many
 * workgroups, with that spin limit and that much dynamic LDS each, so that the give-up path can be
 * provoked.  A negative argument leaves that setting as it is.
 * TEST HOOK, not part of the solver's interface: the settings are one unsynchronised process-wide record (do not
 * call it while another thread is inside mde_lbfgs_dev_step), and the dynamic-LDS attribute it sets on the kernel
 * goes back to 0 only when lds_bytes = 0 is passed again. */
int mde_lbfgs_debug_knobs(int32_t unfused, int32_t blocks, int32_t spins, int32_t lds_bytes);

/* ---- the solver's read-back -------------------------------------------------------------------------
 * device -> pinned-host copy on the stream: [loss | status | statistics board] travels in one copy per
 * objective evaluation [ref: the loop accelerated is optim.py:100-175 + lbfgs.py:390-590, which
 * synchronises >= 12 times per iteration].  (Round 2 also exported mde_capture_* to replay an
 * iteration as one HIP graph; measured slower than the launches it replaced, removed in round 3.) */
int mde_copy_to_host(void* dst_host, const void* src_dev, int64_t bytes, void* stream);

/* ---- one steady-state solver iteration as two calls ----------------------------------------------------
 * The usual L-BFGS iteration accepts its first trial point (t = 1).  Everything such an iteration launches
 * -- direction update (mde_lbfgs_dev_step), trial point retraction(X + dir) (mde_center_step /
 * mde_std_retract_step), objective + gradient (mde_average_distortion), tangent projection + statistics,
 * the read-back -- is described once by mde_turn_desc; mde_turn_enqueue launches it, and mde_turn_wait
 * waits for it, applies the strong-Wolfe acceptance test of the first trial [ref: lbfgs.py:44-253, first
 * pass of the bracketing loop: Armijo with c1 and |g_new.d| <= -c2 g.d] and, when the point is accepted
 * and the caller allows it, launches the NEXT iteration at once -- the host's bookkeeping then runs while
 * the GPU works.  A trial that is not accepted is handed back to the caller's line search unchanged.
 * kind: 0 Centered, 1 Standardized.  X[cur] is the accepted iterate, X[1 - cur] receives the trial. */
typedef struct mde_turn_desc {
  mde_plan* plan;
  const mde_func* func;
  int64_t n;
  int32_t d, kind;
  float* X[2];
  float* g;        /* n*d floats, followed by the loss word (loss_dev) */
  float* g_prev;
  float* dir;
  float* loss_dev;
  double* board;   /* statistics board: [0,8) trial statistics, [16,24) direction statistics */
  double* work;
  int32_t* status;
  mde_lbfgs* lbfgs;
  void* host_dst;            /* pinned mirror of [loss | status | pad | board[0,24)] */
  const void* tail_src;
  int64_t read_bytes;
  const float* host_loss;
  const int32_t* host_status;
  const double* host_board;  /* >= 80 doubles of pinned memory: the last kernel of an iteration writes the 24 mirrored board
                                entries, its sequence number behind them (mde_turn_wait polls that word), and -- in the
                                first 64-byte-aligned 32 doubles at or behind host_board + 32 -- the record again as four
                                lines of seven values + the sequence number, which is what mde_turn_wait reads: a line and
                                its tag reach host memory together, the lines in any order */
  double seq;                /* (library state: sequence number of the iteration enqueued last) */
  double pre_id;             /* (library state: > 0 the L-BFGS step of the iteration after it is queued behind it, -1 that step has run and is pending) */
} mde_turn_desc;
/* f0: the loss at X[cur]; the acceptance test of the trial (c1, c2) is made by the iteration's last kernel,
 * on the device.  allow_pre: also queue the L-BFGS step of the iteration AFTER this one behind it -- its
 * kernels leave at once unless that test accepts the trial (the host's turn-around between two iterations
 * then overlaps with that step); pass 0 when the solve would stop after this iteration anyway. */
int mde_turn_enqueue(mde_turn_desc* T, int32_t cur, float t_prev, double f0, double c1, double c2,
                     int32_t allow_pre, void* stream);
/* out (>= 24 doubles): [0] f_new, [1] accepted, [2] next iteration enqueued, [3] status word,
 * [4,12) trial statistics, [12,20) direction statistics, [20] 1 when the gated L-BFGS step of the NEXT iteration
 * has run (the trial was accepted and the iteration was enqueued with allow_pre) but allow_next = 0 kept that
 * iteration from being launched: the step is then PENDING -- g_prev, the history, dir and out[12,20) are already
 * those of the next iteration, the next mde_turn_enqueue on this descriptor skips its own step (t_prev = 1 is
 * what the pending step used), and mde_lbfgs_dev_step must not be called on the same history in between.
 * eps_pre >= 0: the iteration enqueued here gets
 * allow_pre when the accepted point's gradient norm is above eps_pre; < 0: never.  SYNC (waits for the
 * stream). */
int mde_turn_wait(mde_turn_desc* T, int32_t cur, double f0, int32_t allow_next, double c1, double c2,
                  double eps_pre, double* out, void* stream);

/* ---- weighted isotonic regression (csrc/mde_isotonic.hip) ----
 * out = the nondecreasing sequence that minimises sum_i w_i (y_i - out_i)^2, 0 <= p <= 2^31 - 2 (p = 0: nothing
 * is done).  y finite, w finite and > 0 (NULL: all ones); the caller checks that.  The fit is the left slope of
 * the lower convex hull of the p + 1 points (sum w, sum w (y - ybar)) in double, built by a merge tree over leaves
 * of mde_isotonic_leaf() points: every loop runs at most that many or 32 times whatever the data, nothing
 * spins or waits between workgroups, no atomics; the same bits on every run.  `out` is nondecreasing exactly and
 *   max |out - exact| <= 2^-23 max|y| + 2^-47 (sum_i w_i |y_i|) / min_i w_i.
 * With N = p + 1 points, V = ceil(N / leaf) leaves and up(b) = b rounded up to a multiple of 256, `work` holds
 *   256 + 2 up(8 N) + 2 up(4 N) + 2 up(4 V) + up(8 ceil(V / 2)) + 163840 bytes
 * (W and S in double, two hull buffers, two node-count rows, the tangents of a level, the partial sums of the
 * scans): about 24 bytes a value.  `out` doubles as the buffer of block starts.  ASYNC on `stream`; allocates
 * nothing and reads nothing back. */
int32_t mde_isotonic_leaf(void);
int64_t mde_isotonic_work_bytes(int64_t p);   /* < 0: an MDE_E_* code */
int mde_isotonic(int64_t p, const float* y, const float* w, float* out, void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDE_HIP_H_ */
