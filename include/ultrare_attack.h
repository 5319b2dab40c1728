/*
 * ultrare_attack.h -- the attribute-inference attacker (csrc/attack.hip): part of the C ABI of libultrare_hip.so, included by
 * ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged, as for the other family headers.  A small MLP (one hidden layer of H
 * relu units, or logistic regression for H = 0) is trained by full-batch Adam on m selected rows of a float32 table to tell two
 * groups apart, one parameter set per cross-validation fold, and every row is scored by the fold that held it out; the AUC of such
 * scores is an exact count of pairs.  The arithmetic is stated in numpy in ultrare_amd/attack.py; DESIGN.md 4.30.
 *
 * X (device) float32 rows of stride ld >= d, read in place; rows (device) int32 [m]: the first n1 positions are class 1, the rest
 * class 0; fold_of (device) int32 [m]: the fold that holds a position out (fold f trains on fold_of != f).  1 <= d <= 128,
 * 0 <= H <= 128, 2 <= folds <= 16, folds <= m <= 2^24.  A packed parameter set holds P = H d + 2 H + 1 floats
 * [W1 H x d | b1 H | w2 H | b2], or P = d + 1 floats [w d | b] for H = 0.  stats (device) float32 [folds][2][d] = (mean, 1 / std).
 * The results are a function of the arguments alone: fixed summation orders, no floating-point atomics, equal bytes on any stream.
 * Argument checks come before any HIP call; the memory contract is DESIGN 4.20's (every byte of every output written, nothing read
 * that the call did not write, scratch exactly the sizer's).  Nothing synchronises.
 */
#ifndef ULTRARE_ATTACK_H
#define ULTRARE_ATTACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URE_ATTACK_MAX_D 128
#define URE_ATTACK_MAX_H 128
#define URE_ATTACK_MAX_FOLDS 16
#define URE_ATTACK_MAX_ROWS (1 << 24)
#define URE_ATTACK_CHUNK 256        /* positions per gradient chain (and per workgroup of the training kernel) */
#define URE_AUC_TILE_POS 256        /* positives per workgroup of the pair count, one per lane */
#define URE_AUC_TILE_NEG 1024       /* negatives staged in LDS at a time */

/* Bytes of scratch ure_attack_train needs; -1 for a shape the calls refuse. */
int64_t ure_attack_scratch(int64_t m, int32_t d, int32_t H, int32_t folds);
/* stats[f][0][c], stats[f][1][c] = the mean and 1 / std (0 for a zero-variance column) of column c over the positions with
 * fold_of != f: float64 sums over all m positions in the 256-lane fold's order, a held-out position adding 0.0; rounded once. */
int ure_attack_standardize(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *fold_of, int64_t m, int32_t folds, float *stats,
                           void *stream);
/* `epochs` full-batch Adam epochs of every fold from params0 (device float32 [folds][P]), two launches per epoch on `stream`; the
 * host reads nothing back.  fw (device) float32 [folds][4] = (w_class of class 0, of class 1, m_train, unused); sc (device) float32
 * [epochs][2] = Adam's (lr / (1 - beta1^t), sqrt(1 - beta2^t)).  beta1, beta2, eps, l2: float32 values.  Outputs: params (device)
 * float32 [folds][P], loss (device) float64 [folds][epochs] (an epoch's loss at the parameters it starts from). */
int ure_attack_train(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *fold_of, int64_t m, int64_t n1, int32_t folds, int32_t H,
                     const float *stats, const float *fw, const float *sc, int32_t epochs, float beta1, float beta2, float eps, float l2,
                     const float *params0, float *params, double *loss, void *scratch, int64_t scratch_bytes, void *stream);
/* scores[i] = p of position i under the parameter set and statistics fold_of[i]; fold_of NULL: under set 0 (folds is then the
 * number of sets present, >= 1, and any m >= 1 goes).  A fold_of entry outside [0, folds) gives NaN. */
int ure_attack_score(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *fold_of, int64_t m, int32_t folds, int32_t H,
                     const float *stats, const float *params, float *scores, void *stream);
/* counts[0], counts[1] = the number of pairs (i < n1, j < n2) with scores[pos[i]] > scores[neg[j]] and with equality (-0.0 ==
 * +0.0); *nan_flag = 1 when a selected score is NaN (the counts then say nothing), else 0.  Tiled: one positive per lane, the
 * negatives staged in LDS; integer partial counts per workgroup in scratch, summed by a last launch.  1 <= n1, n2 < 2^31. */
int64_t ure_auc_scratch(int64_t n1, int64_t n2);
int ure_auc_counts(const float *scores, const int32_t *pos, int64_t n1, const int32_t *neg, int64_t n2, int64_t *counts, int32_t *nan_flag, void *scratch,
                   int64_t scratch_bytes, void *stream);
/* counts[0 .. 3] = (tp, fn, tn, fp): a score > thr predicts class 1 (a NaN score does not). */
int ure_confusion_counts(const float *scores, const int32_t *pos, int64_t n1, const int32_t *neg, int64_t n2, float thr, int64_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_ATTACK_H */
