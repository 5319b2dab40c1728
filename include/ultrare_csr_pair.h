/*
 * ultrare_csr_pair.h -- the pair-distance reductions of ultrare_hip.h (ure_pair_*) on a sparse matrix: part of the C ABI of
 * libultrare_hip.so, included by ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged, as for the other CSR entries.
 *
 * A device CSR as ure_csr_cost takes it: row_off [n + 1] int64, col [nnz] int32 (ascending inside a row, no repeats,
 * stored zeros allowed), val [nnz] float32, n rows over n_item columns, 1 <= n, n_item < 2^31; a kernel argument must not be
 * NULL, so an empty matrix passes one unused entry.  The library does not check the column ids.  metric is
 * URE_DIST_EUCLIDEAN, URE_DIST_COSINE or URE_DIST_MANHATTAN; URE_DIST_GIVEN has no CSR form and is refused.
 *
 * D[u, v] is the streamed D of ure_pair_* on the densified n x n_item array BIT FOR BIT, which is never formed: the sum
 * walks the union of the stored columns of rows u and v in ascending column, a column stored in one row only paired with
 * 0.f, with one fmaf / add per term into one float32 accumulator from +0 and the same finishing step (a dense term of two
 * implicit zeros leaves its accumulator unchanged).  A row without a non-zero entry -- an empty one included -- is at
 * cosine distance 1 from every row but itself.  D[u, v] == D[v, u], D[u, u] == 0, no floating-point atomics, and no
 * dependence on the grid, the tile or how query rows are batched: each entry below equals its ure_pair_* namesake on the
 * densified array byte for byte, takes its argument list with (row_off, col, val, n, n_item) in place of (src, n, d), and
 * has its limits, its return codes and its memory contract.  Rows of any length are served: a tile's rows are staged in
 * on-chip memory ure_csr_pair_window() entries per row at a time.
 */
#ifndef ULTRARE_CSR_PAIR_H
#define ULTRARE_CSR_PAIR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Entries of a row staged per item-id window (kCsrPairWindow of csrc/pair_dist.hip; sparse_pair.WINDOW in Python). */
int32_t ure_csr_pair_window(void);
/* ure_pair_knn_scratch's value: n_query * n_nb * 8 bytes per effective split, never n * n_item or n * n; -1 for arguments
 * ure_csr_pair_knn rejects. */
int64_t ure_csr_pair_knn_scratch(int64_t n_query, int64_t n, int32_t n_nb, int32_t splits);
int ure_csr_pair_knn(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric, const int32_t *query,
                     int64_t n_query, int32_t n_nb, int32_t splits, float *dist, int32_t *idx, void *scratch, int64_t scratch_bytes, void *stream);
int ure_csr_pair_rowsum(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric, float *R, void *stream);
int ure_csr_pair_cols(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric, const int32_t *cols,
                      int32_t m, float *out, void *stream);
int ure_csr_pair_label_expsum(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric,
                              const int32_t *label, int32_t k, double *W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_CSR_PAIR_H */
