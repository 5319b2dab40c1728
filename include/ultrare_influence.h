/*
 * ultrare_influence.h -- Newton-step (influence) unlearning of an MF shard (csrc/influence.hip): part of the C ABI of
 * libultrare_hip.so, included by ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged, as for the other CSR entries.  The
 * reference has no such source; the arithmetic is stated in numpy in ultrare_amd/influence.py and the kernels are held to it bit
 * for bit.
 *
 * The graph is ultrare_gcn.h's: off [n_dst + 1] int64 and idx [nnz] int32 of one side (CSR: a user's items; CSC: an item's users)
 * in lightgcn.Graph's fixed order, row / col [nnz] the user and item of a CSR entry, to_csr [nnz] the CSR position of a CSC entry.
 * Tables are row-major [rows][d] float32, directions and results [rows][d] float64, d a power of two in 4 .. 256.
 *
 * Every operation below is ONE float64 operation rounded on its own (no fma; a float32 value is widened exactly first); the chain
 * of a (row, column) stays in one lane and is never split or reordered; a row -- however long -- stays with the one group of
 * d / 4 lanes that owns it.  No floating-point atomics; a row's bytes depend on its own entries and the source tables alone, on
 * any stream.  n_dst, n_src, nnz in 1 .. 2^31 - 1; an index outside its range is read as the nearest valid one (callers check
 * their graphs).  Argument checks come before any HIP call.  Only ure_inf_dot needs scratch memory (ure_inf_dot_scratch).
 * ure_inf_cg_start, _xr, _beta and _p are in-place entries.  Nothing synchronises.
 */
#ifndef ULTRARE_INFLUENCE_H
#define ULTRARE_INFLUENCE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The coefficient pass over the CSR entries k = 0 .. nnz - 1, entries independent, every byte of out [nnz] written.  Lane l of
 * the d / 4 lanes of an entry holds the columns 4 l .. 4 l + 3 and runs p = x_0 y_0, p = fl(p + fl(x_c y_c)) (c = 1, 2, 3); the
 * lane values are added as a balanced tree of adjacent pairs.  Without a direction (P and Q NULL): x = U[row[k]], y = V[col[k]],
 * out[k] = fl(sum - (double)rating[k]) (the residual e).  With one (both given, float64): the lane's chain runs over the four
 * P[row[k]] V[col[k]] products and then the four U[row[k]] Q[col[k]] products, out[k] = the sum (the tangent t). */
int ure_inf_coef(const int32_t *row, const int32_t *col, const float *rating, int64_t nnz, const float *U, const float *V, const double *P,
                 const double *Q, int64_t n_user, int64_t n_item, int32_t d, double *out, void *stream);
/* One walk, one side per call (CSR: map NULL; CSC: map = to_csr).  For row r and column c, over the row's entries k in ascending
 * position from 0.0, q = map ? map[k] : k: acc = fl(acc + fl(a[q] * (double)T[idx[k]][c])), then -- with b and D given (both or
 * neither) -- acc = fl(acc + fl(b[q] * D[idx[k]][c])); out[r][c] = fl(fl(2 acc) + fl(fl(2 reg) * X[r][c])).  A row with
 * active[r] == 0 (active optional, uint8 [n_dst]) or without entries gets +0.0 in every byte and reads none of its entries.
 * a, b [nnz] float64 in CSR order; T [n_src][d] float32 and D [n_src][d] float64 belong to the OTHER side; X, out [n_dst][d]
 * float64 to this one.  out must not overlap any input.  The gradient is a = e, T the other table, no b, reg = l2, X = this
 * side's table widened; the Hessian-vector product a = t, b = e (full curvature) or none (Gauss-Newton), D the other side's
 * direction, reg = l2 + damping, X this side's direction. */
int ure_inf_walk(const int64_t *off, const int32_t *idx, const int32_t *map, const double *a, const float *T, const double *b, const double *D,
                 double reg, const double *X, const uint8_t *active, int64_t n_dst, int64_t n_src, int64_t nnz, int32_t d, double *out,
                 void *stream);
/* out[0] = sum x[i] y[i] over n float64 values (x may be y) in a fixed two-level order: chunk c holds the values 4096 c ..
 * 4096 c + 4095 (the last one fewer); lane t of 256 adds fl(x y) of the chunk's values t, t + 256, ... in ascending order from
 * 0.0 and the 256 lane sums are folded pairwise (w = 128 .. 1: lane t += lane t + w) -- ure_gcn_step_loss's order; the chunk
 * sums are then added in that same order.  scratch: ure_inf_dot_scratch(n) bytes (one float64 per chunk), 0 for n < 1. */
int64_t ure_inf_dot_scratch(int64_t n);
int ure_inf_dot(const double *x, const double *y, int64_t n, void *scratch, int64_t scratch_bytes, double *out, void *stream);
/* Conjugate gradients without a host round trip.  state: 8 float64 in device memory -- [0] rr, [1] pAp, [2] the new rr, [3] the
 * threshold, [4] the flag (0.0 running, 1.0 converged, 2.0 non-positive curvature), [5] alpha, [6] beta, [7] unused; the caller
 * has ure_inf_dot write rr = r . r into state[0] (before _start), pAp = p . Ap into state[1] (before _xr) and the new r . r into
 * state[2] (before _beta).
 * _start: state[3] = fl(fl(tol tol) state[0]); flag = state[0] <= state[3] ? 1 : 0; alpha = beta = 0.
 * _xr:    while the flag is 0 and pAp > 0: alpha = fl(rr / pAp), x[i] = fl(x[i] + fl(alpha p[i])), r[i] = fl(r[i] - fl(alpha Ap[i])).
 * _beta:  while the flag is 0: not pAp > 0 -> flag 2; else beta = fl(state[2] / rr), rr = state[2], rr <= threshold -> flag 1.
 *         Then always log_rr[it] = rr and log_flag[it] = the flag (log_rr float64 [n_log], log_flag int32 [n_log], 0 <= it < n_log).
 * _p:     while the flag is 0: p[i] = fl(r[i] + fl(beta p[i])).
 * Once the flag is set x, r and p keep their bytes in every later call.  x, r, p, Ap: n float64 each, no overlap. */
int ure_inf_cg_start(double *state, double tol, void *stream);
int ure_inf_cg_xr(const double *state, double *x, double *r, const double *p, const double *Ap, int64_t n, void *stream);
int ure_inf_cg_beta(double *state, double *log_rr, int32_t *log_flag, int64_t it, int64_t n_log, void *stream);
int ure_inf_cg_p(const double *state, double *p, const double *r, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_INFLUENCE_H */
