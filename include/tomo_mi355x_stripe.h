/* tomo_mi355x_stripe.h -- the two launches PDHG's stripe variable adds to include/tomo_mi355x.h (RecToolsIRCuPy.PDHG with
 * _data_["stripe_lambda"]; docs/kernels/pdhg.md, "The stripe variable").  Same library, same conventions: C linkage, float32
 * device arrays, every scalar a float32 value computed by the caller, 0 / TOMO_E_* return codes with tomo_last_error,
 * asynchronous on the stream passed in.  TOMO_ABI_VERSION stays what it is: the header adds symbols and changes none.
 *
 * Why a header of its own: tests/test_stream_coverage.py and tests/test_host_logic.py pin the main header's prototypes to
 * their tables by count and by name, and this addition was not to edit them; tests/test_pdhg_stripe_surface.py holds this
 * header to the same two rules (every name bound in _lib.EXT_SIGNATURES and exported by both libraries, every prototype with
 * a stream run on a side stream by tests/test_gpu_pdhg_stripe.py).  A later change that may edit those tests folds this
 * file into the main header and EXT_SIGNATURES into SIGNATURES.
 *
 * The problem: min_{x, s} F(A x + S s; b) + lambda R(x) + mu |s|_1, s[z][u] one offset per detector pixel, (S s)[z][a][u] =
 * s[z][u].  The sinogram is [nz][na][nu], u fastest; the angles are cut into n_seg = ceil(na / TOMO_PDHG_STRIPE_SEG)
 * segments of TOMO_PDHG_STRIPE_SEG rows, so that the sum of y over the angles is deterministic and still parallel along them.
 * No reference counterpart: tests/_pdhg_stripe_oracle.py restates both launches in numpy and they equal its float32 form
 * bit for bit (one rounding per operation, no FMA contraction).
 *
 *   tomo_pdhg_sino_dual_stripe: step 2 of a PDHG iteration with the stripe variable.  Per sample e = r + sbar[z][u], then
 *     the prox of tomo_pdhg_sino_dual with e in place of r (TOMO_PDHG_LS, TOMO_PDHG_L1, TOMO_PDHG_KL), y in place; and
 *     part[k][z][u] = the sum of the new y[z][a][u] over the rows a of segment k, ascending from +0.  sigma_dev NULL: the
 *     scalar step `sigma`; else one step per sample (an array like y; `sigma` is not read).  About 16 B per sample (20 with
 *     sigma_dev).  16-byte accesses where nu % 4 == 0 and y, r, b (and sigma_dev) are 16-byte aligned, scalar ones otherwise.
 *     TOMO_E_INVALID: an unknown term, nz, na or nu below 1, a non-positive sigma with sigma_dev NULL, NULL, y or part
 *     aliasing another array of the call.
 *   tomo_pdhg_stripe_update: step 6.  Per (z, u): c = the sum of part[k][z][u] over k ascending from +0; w = s - tau_s c;
 *     s' = w > theta ? w - theta : (w < -theta ? w + theta : +0); sbar <- (s' + s') - s; s <- s'.  `na` is the number of
 *     angles the partial sums were taken over (it fixes n_seg).  TOMO_E_INVALID: nz, na or nu below 1, a non-positive tau_s, a
 *     negative theta, NULL, aliasing arrays. */
#ifndef TOMO_MI355X_STRIPE_H
#define TOMO_MI355X_STRIPE_H

#include "tomo_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOMO_PDHG_STRIPE_SEG 64

int tomo_pdhg_sino_dual_stripe(float *y_dev, const float *r_dev, const float *b_dev, const float *sigma_dev,
                               const float *sbar_dev, float *part_dev, int nz, int na, int nu, int fidelity, float sigma,
                               void *stream);
int tomo_pdhg_stripe_update(float *s_dev, float *sbar_dev, const float *part_dev, int nz, int na, int nu, float tau_s,
                            float theta, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TOMO_MI355X_STRIPE_H */
