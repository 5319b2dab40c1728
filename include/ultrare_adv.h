/*
 * ultrare_adv.h -- adversarial attribute unlearning against the probe of ultrare_attack.h (csrc/adv.hip): part of the C ABI of
 * libultrare_hip.so, included by ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged, as for the other family headers.  The
 * one entry is the other half of the game ultrare_attack.h plays: the gradient of the probe's loss with respect to its INPUT rows.
 * The arithmetic is stated in numpy in ultrare_amd/adv_unlearn.py (input_grad_ref); DESIGN.md 4.31.
 *
 * X, ld, d, rows, fold_of, m, n1, folds, H, stats, params and fw are ultrare_attack.h's: 1 <= d <= 128, 0 <= H <= 128,
 * 1 <= folds <= 16, 1 <= m <= 2^24, 0 <= n1 <= m; params (device) float32 [folds][P], stats (device) float32 [folds][2][d], fw
 * (device) float32 [folds][4] = ure_attack_train's (w_class of class 0, of class 1, m_train, unused).
 * The result is a function of the arguments alone: fixed summation orders, no floating-point atomics, equal bytes on any stream.
 * Argument checks come before any HIP call; every byte of the outputs is written exactly once, there is no scratch.  Nothing
 * synchronises.
 */
#ifndef ULTRARE_ADV_H
#define ULTRARE_ADV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URE_ADV_RUN 256         /* positions of ONE fold per workgroup */

/* grad[i][c] (device float32 [m][d], dense) = the derivative, with respect to column c of the selected row i, of the row's own term
 * w_class[f][y_i] * (the cross-entropy of p_i against target[y_i]) under the parameter set and statistics of f = fold_of[i], the
 * fold that held position i out (fold_of NULL: set 0); y_i = 1 for i < n1.  (target0, target1), two finite floats (NaN and the
 * infinities are refused): (0, 1) is the attacker's own loss, (0.5, 0.5) the confusion target.  No division by m_train, no gradient through the statistics.  p_out (device float32 [m],
 * or NULL) receives p_i, the value ure_attack_score gives.
 *
 * The plan: perm (device int32 [m]) lists the positions grouped by fold and fold_off (device int32 [folds + 2]) the ascending
 * offsets of the groups into it: group f < folds holds the positions with fold_of == f, group `folds` those whose fold_of lies
 * outside [0, folds).  Both are required with fold_of and ignored (NULL allowed) without it.  A workgroup owns up to URE_ADV_RUN
 * consecutive entries of one group.  The plan decides who works on a position, fold_of what it is given: a position met in a
 * group other than fold_of's (the last group always) gets a NaN row and a NaN p.  The kernel clamps the offsets to [0, m] and
 * skips a perm entry outside [0, m), so a bad plan cannot make it write out of bounds; a plan that is no permutation leaves
 * positions unwritten or written twice.  The host cannot check device data: a correct plan is the caller's duty. */
int ure_adv_input_grad(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *fold_of, int64_t m, int64_t n1, int32_t folds, int32_t H,
                       const float *stats, const float *params, const float *fw, float target0, float target1, float *grad, float *p_out,
                       const int32_t *perm, const int32_t *fold_off, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_ADV_H */
