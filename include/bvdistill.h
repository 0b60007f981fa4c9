/* libbvdistill — C ABI of the knowledge-distillation loss kernels for the MI355X (gfx950).
 *
 * A second in-tree library next to libbvhip (include/bvhip.h), with the same conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (no hidden allocation); tensors are row-major and
 *     densely packed: a logit matrix is fp32 [n][C], exactly n * C floats, nothing is read or written past them;
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns immediately: 0 = ok,
 *     <0 = error (BVD_ERR_*); the message is available from bv_distill_last_error().  No call synchronises;
 *   - thread-safe per stream; the library keeps NO process-global state besides the (thread-local) last-error string.
 *
 * It replaces the jax.numpy lowering of the reference's distillation loss and of the measurements its trainer
 * logs: evaluators/proj/distill/distance.py:35-67 (`dist`), utils.py:276-281 (`softmax_xent(..., kl=True)`),
 * trainers/proj/distill/distill.py:232-233 (entropy), :242-245 (loss per teacher), :346-351 (teacher ensemble);
 * paths relative to big_vision/ in the reference tree.
 *
 * n = rows of this call, n_global >= n = rows of the whole (data-parallel) batch: means are over n_global, so
 * per-rank sums are partial sums (all-reduce SUM), as with bv_softmax_xent.
 */
#ifndef BVDISTILL_H_
#define BVDISTILL_H_

#ifdef __cplusplus
extern "C" {
#endif

#define BVDISTILL_VERSION 1

/* error codes (the values of BV_ERR_* in bvhip.h) */
#define BVD_OK 0
#define BVD_ERR_INVALID_ARG (-1)
#define BVD_ERR_UNSUPPORTED (-2)
#define BVD_ERR_HIP (-3)

const char* bv_distill_last_error(void);
int bv_distill_version(void);

/* kinds of distance.py:35-67 */
#define BVD_KIND_L2 0
#define BVD_KIND_EUCLIDEAN 1
#define BVD_KIND_KL 2
#define BVD_KIND_HARD 3
#define BVD_KIND_LOGSOFTMAX_EUCLIDEAN 4
#define BVD_KIND_AGREE 5
#define BVD_KIND_COUNT 6

/* One (student, teacher) pair, one launch, one workgroup per row.  With d = s - T, p = softmax, lp = log_softmax:
 *   kind                   value d_i of row i                                          d value / d s_j
 *   L2                     sum d^2                                                     2 d_j
 *   EUCLIDEAN              sqrt(sum d^2 + eps)                                         d_j / value
 *   KL                     t^2 [-sum y lp(s/t) + sum y log(max(y, 1e-8))], y = p(T/t)  t (p(s/t)_j - y_j)
 *   HARD                   the same bracket with t = 1 and y = (1 - ls) onehot(a)      p(s)_j - y_j
 *                          + ls / (C - 1) (1 - onehot(a)), a = FIRST index of max T
 *   LOGSOFTMAX_EUCLIDEAN   sqrt(sum e^2 + eps), e = lp(s) - lp(T)                      (e_j - p(s)_j sum_c e_c) / value
 *   AGREE                  1 if a is among the student's top k, i.e.                   (none)
 *                          #{c: s_c > s_a} + #{c < a: s_c == s_a} < k (lax.top_k, ties to the lower index), else 0
 * Arguments a kind does not use are ignored (t: KL; ls: HARD; eps: the two square roots; k: AGREE).
 *   student, teacher  fp32 [n][C], read: n * C floats each.
 *   per_row           fp32 [n] or NULL: per_row[i] = d_i (written, n floats).
 *   loss_sum          fp64 [1] or NULL: loss_sum[0] += sum_i d_i / n_global (one atomic add per row).
 *   dstudent          fp32 [n][C] or NULL: d(sum_i d_i / n_global) / d student; accumulate = 0 writes, accumulate = 1
 *                     adds to what is there (several teachers).  n * C floats, each written once.
 * For C <= 4096 every logit is read from memory once (the row lives in registers across all phases), with 16-byte
 * accesses when C % 4 == 0 and student, teacher and dstudent are 16-byte aligned and 4-byte accesses otherwise; any
 * alignment of fp32 data is accepted.  For C > 4096 every phase re-reads the row (4 to 6 reads of each logit) and all
 * accesses are 4-byte ones whatever the alignment: a fallback that computes the same values, not a tuned path.
 * BVD_ERR_INVALID_ARG: n <= 0, C <= 0, n_global < n, unknown kind, NULL student / teacher, KL with t <= 0, HARD with
 * C = 1 and ls != 0, AGREE with k < 1 or a non-NULL dstudent, eps < 0. */
int bv_distill_dist(int kind, const float* student, const float* teacher, float* per_row, double* loss_sum,
                    float* dstudent, int accumulate, int n, int C, int n_global, float t, float ls, float eps, int k,
                    void* stream);

/* Entropy of softmax(logits) per row, -sum_c p_c log p_c (distill.py:232-233).  logits fp32 [n][C] (n * C floats read);
 * per_row fp32 [n] or NULL (written); sum fp64 [1] or NULL: sum[0] += sum_i H_i / n_global. */
int bv_distill_entropy(const float* logits, float* per_row, double* sum, int n, int C, int n_global, void* stream);

/* probs (+)= weight * softmax(logits) per row: the teacher ensemble in probability space (distill.py:346-351, with
 * weight = 1 / #teachers).  logits, probs fp32 [n][C]; accumulate = 0 writes probs, 1 adds to it; n * C floats each. */
int bv_distill_softmax_acc(const float* logits, float* probs, float weight, int accumulate, int n, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BVDISTILL_H_ */
