/*
 * ultrare_wmf.h -- weighted matrix factorisation for implicit feedback (csrc/wmf.hip): part of the C ABI of libultrare_hip.so, included
 * by ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged, as for the other family headers.  A half sweep of implicit ALS (Hu,
 * Koren, Volinsky 2008) is the Gram matrix of the whole fixed table (ure_gram) and one weighted ridge system per row that adds it
 * (ure_wridge_rows); the arithmetic is stated in numpy in ultrare_amd/wmf.py; DESIGN.md 4.32.
 *
 * F (device) float32 [n][d], d a power of two in 4 .. 128, of which the first k columns count (1 <= k <= d).  A Gram matrix G0 is the
 * packed upper triangle, row-major: k (k + 1) / 2 doubles, entry (a, b), a <= b, at a k - a (a - 1) / 2 + b - a.
 * The results are a function of the arguments alone: fixed summation orders, no floating-point atomics, equal bytes on any stream
 * and however the workgroups are scheduled.  Argument checks come before any HIP call; the memory contract is DESIGN 4.20's (every byte of
 * every output written, nothing read that the call did not write, scratch exactly the sizer's).  Nothing synchronises.
 */
#ifndef ULTRARE_WMF_H
#define ULTRARE_WMF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URE_GRAM_CHUNK 256          /* rows per inner chain of ure_gram (and per partial triangle in its scratch) */

/* Bytes of scratch ure_gram needs: ceil(n / 256) partial triangles; -1 for n outside 1 .. 2^31 - 1 or k outside 1 .. 128. */
int64_t ure_gram_scratch(int64_t n, int k);
/* G0[a][b] = sum_i F[i][a] F[i][b] (a <= b < k) in float64, a two-level chain: inside a chunk of 256 consecutive rows in ascending row
 * order from 0.0, then the chunk sums in ascending chunk order starting from the first.  Products of float32 values are exact in
 * float64, so this is a BIT contract (wmf.gram_ref).  Two launches on `stream`: the chunk partials into scratch, then their fold. */
int ure_gram(const float *F, int64_t n, int d, int k, double *G0, void *scratch, int64_t scratch_bytes, void *stream);

/* ure_ridge_rows (ultrare_hip.h) with a confidence per entry and a Gram matrix added to every system.  Segment s, entries j in CSR
 * order, n_s of them, f_j = (double)F[idx[j]][0:k]:
 *   G = G0 + sum_j wg[j] f_j f_j^T + (l2 + l2_n n_s) I,  b = sum_j wb[j] f_j,  X[s][0:k] = G^-1 b (Cholesky, float64, rounded once).
 * The term for (a, b) is fma(wg[j] f_a, f_b, acc); G0 joins as acc + G0[a][b], then + ridge on the diagonal; G0 NULL adds nothing, and
 * with wg = 1, wb = val the bytes are ure_ridge_rows's.  off, idx, m, order, X, status, the empty segment, the failed segment and
 * the scratch (0 bytes; -1 for m < 0 or k outside 1 .. 128; scratch may be NULL) are ure_ridge_rows's; wg, wb (device) float32 [nnz]. */
int64_t ure_wridge_rows_scratch(int64_t m, int k);
int ure_wridge_rows(const float *F, int64_t n_fixed, int d, int k, const int64_t *off, const int32_t *idx, const float *wg, const float *wb,
                    int64_t m, const int32_t *order, const double *G0, double l2, double l2_n, float *X, int32_t *status, void *scratch,
                    int64_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_WMF_H */
