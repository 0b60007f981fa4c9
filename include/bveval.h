/* libbveval — C ABI of the classification-evaluation kernel for the MI355X (gfx950).
 *
 * A third in-tree library next to libbvhip (include/bvhip.h) and libbvdistill (include/bvdistill.h), with the same
 * conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (no hidden allocation); matrices are row-major and densely
 *     packed: a logit matrix is fp32 [n][C], exactly n * C floats, nothing is read or written past them;
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns immediately: 0 = ok,
 *     <0 = error (BVE_ERR_*); the message is available from bv_eval_last_error().  No call synchronises;
 *   - thread-safe per stream; the library keeps NO process-global state besides the (thread-local) last-error string.
 *
 * It replaces the jax.numpy lowering of the reference's classification evaluator, evaluators/classification.py:37-53
 * (`_eval_fn`: the label mask, the loss, the argmax, the label gathered at the argmax and the three sums), with the
 * two losses it is configured with: utils.py:236-243 (`sigmoid_xent`) and utils.py:276-281 (`softmax_xent`), both at
 * reduction=False; paths relative to big_vision/ in the reference tree.
 */
#ifndef BVEVAL_H_
#define BVEVAL_H_

#ifdef __cplusplus
extern "C" {
#endif

#define BVEVAL_VERSION 1

/* error codes (the values of BV_ERR_* in bvhip.h) */
#define BVE_OK 0
#define BVE_ERR_INVALID_ARG (-1)
#define BVE_ERR_UNSUPPORTED (-2)
#define BVE_ERR_HIP (-3)

const char* bv_eval_last_error(void);
int bv_eval_version(void);

/* losses of utils.py, by `loss_name` of classification.py:43 */
#define BVE_LOSS_SOFTMAX_XENT 0
#define BVE_LOSS_SIGMOID_XENT 1
#define BVE_LOSS_COUNT 2

/* One batch of classification.py:37-53, one launch.  With l = logits[i], y = labels[i] (rows of C floats):
 *   m_i    = mask[i] * max_c y_c         a literal product: a row of all-zero labels drops out (:41); mask NULL = ones
 *   loss_i = SOFTMAX_XENT   -sum_c y_c log_softmax(l)_c, evaluated as (sum_c y_c) lse(l) - sum_c y_c l_c
 *            SIGMOID_XENT   -sum_c [y_c log_sigmoid(l_c) + (1 - y_c) log_sigmoid(-l_c)],
 *                           log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|))
 *   a_i    = argmax_c l_c with jnp.argmax rules: ties go to the lowest index, a NaN counts as the maximum and the
 *            first NaN wins
 *   acc[0] += sum_i y[i][a_i] m_i   (ncorrect)    acc[1] += sum_i loss_i m_i   (loss)    acc[2] += sum_i m_i   (nseen)
 * Non-finite logits behave as in the reference: a NaN or +inf logit makes loss_i (and so acc[1]) NaN, whatever m_i.
 *   logits, labels  fp32 [n][C], read: n * C floats each, each ONCE, for any C: one streaming pass keeps a running
 *                   maximum with a rescaled running sum of exponentials (online log-sum-exp), sum y l, sum y, max y and
 *                   the best (value, index, label) per lane and merges the lanes afterwards.  16-byte loads when
 *                   C % 4 == 0 and both matrices are 16-byte aligned, 4-byte loads otherwise; any alignment of fp32
 *                   data is accepted.
 *   mask            fp32 [n] or NULL: n floats read.
 *   acc             fp64 [3] or NULL: 24 bytes, added to with three fp64 atomic adds per workgroup.  The products with
 *                   m_i and the sums over rows are formed in fp64; the order of the atomic adds (and so of the sum) is
 *                   unspecified: with fp64 partial sums of fp32 values that moves the result by ~1e-16 relative, far
 *                   below every tolerance it is held to.
 *   row_loss        fp32 [n] or NULL: row_loss[i] = loss_i, NOT multiplied by m_i (n floats written).
 *   row_top1        int32 [n] or NULL: row_top1[i] = a_i (n ints written).
 * Row mapping: C <= 1024 (BVE_WAVE_ROW_MAX_C): one 64-lane wave per row, four rows per 256-lane workgroup;
 * C > 1024: one 256-lane workgroup per row.  At most 2048 workgroups are launched; they stride over the rows.
 * BVE_ERR_INVALID_ARG: n <= 0, C <= 0, unknown loss_kind, NULL logits or labels, acc, row_loss and row_top1 all NULL. */
#define BVE_WAVE_ROW_MAX_C 1024
int bv_eval_classify(int loss_kind, const float* logits, const float* labels, const float* mask, double* acc,
                     float* row_loss, int* row_top1, int n, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BVEVAL_H_ */
