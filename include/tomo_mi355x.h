/*
 * tomo_mi355x.h -- C-ABI of libtomo_mi355x.so: the MI355X (gfx950) drop-in for the
 * ordered-subsets FISTA / ADMM hot path of ToMoBAR (parallel-beam 3D forward / back
 * projection, data-fidelity gradient, TV proximal operators and the element-wise glue).
 *
 * Conventions
 *   - every pointer named *_dev is a caller-owned DEVICE pointer to C-contiguous float32;
 *     the library owns only opaque contexts (geometry tables, grow-only scratch arena);
 *   - volume  layout [nz][n][n]   (z, y, x)   -- astra.geom_size(vol_geom),  astra_base.py:215-222,547
 *   - sinogram layout [nz][na][nu] (detY, angles, detX)                   -- dicts.py:50, astra_base.py:247-252,592
 *   - voxel (ix,iy,iz) centre at (ix-n/2+1/2, iy-n/2+1/2, iz-nz/2+1/2), unit voxels, no axis flips;
 *     detector pixel iu at signed offset cor + iu - nu/2 + 1/2 along u=(cos t, sin t, 0); rays (sin t, -cos t, 0)
 *     (tomobar/supp/funcs.py:45-65); detector row iv == volume slice iz;
 *   - every entry point is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     unless it returns a scalar to the host (tomo_norm2, tomo_max);
 *   - return value 0 = ok; otherwise a TOMO_E_* code and tomo_last_error() (thread-local) describes it.
 *
 * Each entry point cites the reference interface it replaces (paths relative to /root/reference).
 */
#ifndef TOMO_MI355X_H
#define TOMO_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* raised whenever a signature changes or an entry point is added (tomobar_amd/_lib.py checks it at load).  The three
 * tomo_diff4th* entry points joined version 10 without a raise: tests/test_ndf_oracle.py pins the number 10, and _lib.py
 * binds every symbol by name at load, so a library without them is refused all the same.  The three tomo_llt_rof* entry
 * points joined it the same way, for the same reason.  So did the four tomo_wavelet_* entry points, and tomo_halo_pack2 /
 * tomo_halo_pull2 with the four tomo_ipc_region_* entry points, and tomo_nltv_scratch_bytes, tomo_patch_select and
 * tomo_nltv, and the five entry points of the private volume layout (TOMO_VOLUME_ZQUAD below), and the four tomo_pdhg_* entry
 * points (tests/test_matched_bp_oracle.py pins the number 10 as well), and the five tomo_spdhg_* entry points, and the four
 * entry points of PDHG's diagonal preconditioner (tomo_pdhg_diag_*, tomo_pdhg_*_diag), and the five tomo_pdhg_tgv_* entry
 * points, and tomo_pdhg_sino_dual_stripe and tomo_pdhg_stripe_update. */
#define TOMO_ABI_VERSION 10

enum {
    TOMO_OK = 0,
    TOMO_E_INVALID = 1,  /* bad argument: maps to ValueError in the Python layer */
    TOMO_E_RUNTIME = 2,  /* HIP runtime failure */
    TOMO_E_NOMEM = 3,
    TOMO_E_NODEVICE = 4  /* no usable gfx950 device: the product path fails loudly, there is no CPU fallback */
};

/* ctx flags */
#define TOMO_FLAG_LERP8 1u /* quantise interpolation weights to 8 fractional bits (NVIDIA texture-unit emulation) */

/* data fidelity selector of tomobar/data_fidelities.py:28-39;
 * TOMO_FID_RATIO = b / max(Ax, 1e-8), the OSEM ratio of methodsIR_CuPy.py:648-650 */
enum { TOMO_FID_LS = 0, TOMO_FID_PWLS = 1, TOMO_FID_KL = 2, TOMO_FID_RATIO = 3 };

typedef struct tomo_ctx tomo_ctx;

/* per-angle geometry record (host-visible copy of the device table) */
typedef struct {
    float cs, sn;   /* (float)cos(theta), (float)sin(theta) */
    float cor;      /* horizontal CoR offset */
    float slope;    /* FP: d(interp coordinate)/d(step) */
    float inv;      /* FP: 1/sin (x-stepping) or 1/cos (y-stepping) */
    float scale;    /* FP: ray length per step */
    int32_t dirx;   /* FP: 1 = step along x / interpolate along y */
    int32_t src;    /* index into the full sinogram's angle axis */
} tomo_angle_t;

int tomo_abi_version(void);
/* "shipped" (libtomo_mi355x.so) or "dev" (libtomo_mi355x_dev.so, built with -DTOMO_DEV_VARIANTS for tests / tools) */
const char *tomo_build_flavour(void);
const char *tomo_last_error(void);
int tomo_device_count(int *count);

/* ---------------------------------------------------------------- context / geometry
 * Replaces AstraTools3D.__init__ -> AstraBase._set_vol3d_geometry (astra_base.py:215-222),
 * _set_gpu_projection3d_parallel_geometry (:244-255), _setOS_indices (:195-209) and
 * _set_projection3d_OS_parallel_geometry (:287-308); geometry vectors of supp/funcs.py:45-65.
 * angles_host [na] radians (float64).  cor_host: cor_stride==0 -> one scalar; ==1 -> [na];
 * ==2 -> [na][2] (horizontal, vertical) where the vertical component must be 0.
 * Nothing is created per call afterwards (the reference re-creates an ASTRA projector per call,
 * astra_base.py:538-545,586-604). */
int tomo_ctx_create(int device, int nz, int n, int nu, int na, const double *angles_host,
                    const double *cor_host, int cor_stride, int os_number, unsigned flags,
                    tomo_ctx **out);
int tomo_ctx_destroy(tomo_ctx *ctx);
int tomo_ctx_os_number(const tomo_ctx *ctx);
int tomo_ctx_num_bins(const tomo_ctx *ctx);                       /* AstraBase.NumbProjBins */
/* AstraBase.newInd_Vec, [os_number][num_bins] int64, zero-filled tail (astra_base.py:199-209) */
int tomo_ctx_newind_table(const tomo_ctx *ctx, int64_t *out_host);
/* subset = -1 -> all angles.  Size after the one-element trim of methodsIR_CuPy.py:454-456. */
int tomo_ctx_subset_size(const tomo_ctx *ctx, int subset);
int tomo_ctx_angle_table(const tomo_ctx *ctx, int subset, tomo_angle_t *out_host, int capacity);
/* release the context's scratch arena (cp._default_memory_pool.free_all_blocks(), methodsIR_CuPy.py:425) */
int tomo_ctx_release_scratch(tomo_ctx *ctx);
/* diagnostics: which kernel form the LAST tomo_fp3d* ("fp") / tomo_bp3d* ("bp") call on this context took, e.g.
 * "y:whole-row(1024 threads, 3 passes, 3 rows/chunk) ...".  The library also prints one stderr warning per process when
 * a slow fallback form is taken.  (No reference counterpart: ASTRA picks its kernels internally, astra_base.py:554,601.) */
const char *tomo_ctx_kernel_path(const tomo_ctx *ctx, const char *op);

/* ---------------------------------------------------------------- projector pair
 * tomo_fp3d  replaces AstraBase.runAstraProj3DCuPy  (astra_base.py:560-606, direct_FP3D :601)
 *            reached through AstraTools3D._forwprojCuPy/_forwprojOSCuPy (astra_tools3d.py:78-86).
 * tomo_bp3d  replaces AstraBase.runAstraBackproj3DCuPy (astra_base.py:518-558, direct_BP3D :554)
 *            reached through _backprojCuPy/_backprojOSCuPy (astra_tools3d.py:102-110).
 * sino_dev is [nz][subset_size][nu]; both outputs are fully overwritten.
 * Scratch: tomo_fp3d* keeps an in-plane transposed copy of the volume in the context (nz*n*n floats, tomo_ctx_release_scratch);
 * tomo_bp3d* (every form, fused epilogues included) re-lays a PLANAR sinogram quad-interleaved -- one streaming pass -- into a
 * scratch arena of this (device, stream) that is as large as the sinogram (4*ceil(nz/4)*subset_size*nu floats, grow-only, freed
 * by tomo_release_scratch): its kernel stages that layout by LDS-DMA, which is worth 7-8 x the pass.  Sinograms beyond 16 GiB,
 * or a device that cannot provide the arena (remembered, never asked again), take the planar staging instead: slower, same bits. */
int tomo_fp3d(tomo_ctx *ctx, int subset, const float *vol_dev, float *sino_dev, void *stream);
int tomo_bp3d(tomo_ctx *ctx, int subset, const float *sino_dev, float *vol_dev, void *stream);

/* ---------------------------------------------------------------- fused data-fidelity gradient
 * tomo_fp3d_residual: res = w_s (.) (A_s x - b_s)  [LS/PWLS]   or   1 - b_s / max(A_s x, 1e-8)  [KL]
 *   i.e. data_fidelities.py:28-39 with the subset gather b[:, indVec, :] of methodsIR_CuPy.py:457
 *   done by index inside the kernel.  b_dev / w_dev are FULL sinograms [nz][na][nu] by default;
 *   `gathered` bit 0 / bit 1 says that b_dev / w_dev is already the subset's [nz][subset_size][nu]
 *   (the form grad_data_term receives, data_fidelities.py:7-14).  w_dev may be NULL (LS).
 *   res_dev is [nz][subset_size][nu]. */
#define TOMO_GATHERED_B 1
#define TOMO_GATHERED_W 2
int tomo_fp3d_residual(tomo_ctx *ctx, int subset, const float *vol_dev, const float *b_dev,
                       const float *w_dev, int gathered, int fidelity, float *res_dev, void *stream);

/* ---------------------------------------------------------------- robust data terms: Huber and Student's t
 * Listed as supported data fidelities in docs/source/introduction/about.rst:38 and driven by _data_["huber_threshold"] /
 * _data_["studentst_threshold"] in Demos/methods_IR_legacy/DemoFISTA_artifacts2D.py:197,263,307,348 -- keys of the reference's
 * removed RecToolsIR class; this reference version has no implementation (supp/dicts.py:85-88), so parity is formula-level
 * (oracle/tomo_oracle.py fista(..., huber=, studentst=)), UNPINNED.  Both re-weight the (weighted) residual r before A^T:
 *   TOMO_ROBUST_HUBER     : r <- (delta / |r|) r  where |r| > delta   (gradient of the Huber function of threshold delta)
 *   TOMO_ROBUST_STUDENTST : r <- (2 / (delta^2 + r^2)) r              (gradient of log(delta^2 + r^2), [KAZ1_2017])
 * tomo_fp3d_residual_robust = tomo_fp3d_residual (LS / PWLS) with the re-weighting in the same epilogue (either residual
 * layout); tomo_sino_robust re-weights an existing residual of `count` floats in place (ring-term / vertical-CoR paths). */
enum { TOMO_ROBUST_NONE = 0, TOMO_ROBUST_HUBER = 1, TOMO_ROBUST_STUDENTST = 2 };
int tomo_fp3d_residual_robust(tomo_ctx *ctx, int subset, const float *vol_dev, const float *b_dev, const float *w_dev,
                              int gathered, int fidelity, int robust, float delta, float *res_dev, void *stream);
int tomo_sino_robust(float *res_dev, size_t count, int robust, float delta, void *stream);

/* ---------------------------------------------------------------- ring-artefact data terms (BASELINE configs[4])
 * Not in this reference version (supp/dicts.py:85-88 accepts LS / PWLS / KL only); they are documented for its removed
 * RecToolsIR class: keys ringGH_lambda / ringGH_accelerate (Group-Huber) and data fidelity "SWLS" + beta_SWLS
 * (docs/source/tutorials/real_data_recon.rst:100-151), models in docs/Kazantsev_CT_20.pdf Table III:
 *   Group-Huber  min_s 1/2 ||s - L^T r||^2 + lambda ||s||_1,  L = (I (x) 1)/sqrt(m2): one offset per detector pixel,
 *                constant over the angles; SWLS: W_s = W - W 1 (1^T W 1 + beta)^-1 1^T W per detector pixel.
 * Parity for these entry points is formula-level only (oracle/tomo_oracle.py fista(..., ring=...)).
 * tomo_fp3d_residual_ring: res = (A_s x - b_s) + ring_scale * r_x[z,u]   (r_x: [nz][nu], broadcast over the angles)
 * tomo_ring_gh_reduce    : vec[z,u] = sum_a res[z,a,u] (ascending a); r_out = r_x - l_inv*vec; then, if w_full_dev is
 *                          given, res[z,a,u] *= w_full[z, src[a], u] in place (PWLS weights after the offset step)
 * tomo_swls_apply        : res_a <- w_a res_a - w_a (sum_a w_a res_a)/(sum_a w_a + beta) per detector pixel
 * tomo_ring_gh_update    : r <- soft(r, lambda); r_x = r + beta (r - r_old); r_old <- r     (count = nz*nu)
 * src_dev: int32 [na_s], the subset's indices into the full sinogram's angle axis. */
int tomo_fp3d_residual_ring(tomo_ctx *ctx, int subset, const float *vol_dev, const float *b_full_dev,
                            const float *ring_dev, float ring_scale, float *res_dev, void *stream);
int tomo_ring_gh_reduce(float *res_dev, const float *w_full_dev, const int *src_dev, int nz, int na_s, int na_full,
                        int nu, const float *rx_dev, float l_inv, float *r_out_dev, void *stream);
int tomo_swls_apply(float *res_dev, const float *w_full_dev, const int *src_dev, int nz, int na_s, int na_full, int nu,
                    float beta, void *stream);
int tomo_ring_gh_update(float *r_dev, float *r_old_dev, float *rx_dev, float lambda, float beta, size_t count,
                        void *stream);

/* ---------------------------------------------------------------- vertical centre-of-rotation component
 * CenterRotOffset may be [angles, 2] = (horizontal, vertical) offsets (supp/funcs.py:52-55).  The context takes the
 * horizontal components; a vertical component moves the detector of angle a by shift[a] rows, which for parallel rays is a
 * per-angle 2-tap resampling of the detector rows (zero outside): A_v = R(+shift) A, A_v^T = A^T R(-shift).
 * tomo_shift_rows: out[r,a,:] = (1-w) in[r+k,a,:] + w in[r+k+1,a,:], k + w = sign*shift[a], k = floor (shift_dev: float32 [na];
 * the weight does not depend on the row, so a z-slab with ghost rows resamples exactly as the whole detector does).
 * tomo_sino_residual: the residual of data_fidelities.py:28-39 on an already projected subset (the fused
 * tomo_fp3d_residual cannot resample between projector and residual; ``gathered`` as there).  Not used when no vertical component is given. */
int tomo_shift_rows(const float *in_dev, float *out_dev, int nz, int na, int nu, const float *shift_dev, float sign,
                    void *stream);
int tomo_sino_residual(const float *ax_dev, const float *b_full_dev, const float *w_full_dev, const int *src_dev, int nz,
                       int na_s, int na_full, int nu, int gathered, int fidelity, float *res_dev, void *stream);
/* tomo_sino_add_ring: res[z,a,u] += ring_scale * ring[z,u] -- the Group-Huber offsets on a residual formed by
 * tomo_sino_residual (the pair replaces tomo_fp3d_residual_ring when a vertical component sits between projector and residual). */
int tomo_sino_add_ring(float *res_dev, const float *ring_dev, float ring_scale, int nz, int na_s, int nu, void *stream);

/* tomo_bp3d_fista: x_out = P+( x_t - l_inv * A_s^T res )            methodsIR_CuPy.py:463-468
 *   nonneg != 0 applies the max(.,0) projection.  x_out may alias x_t. */
int tomo_bp3d_fista(tomo_ctx *ctx, int subset, const float *res_dev, const float *xt_dev,
                    float *xout_dev, float l_inv, int nonneg, void *stream);
/* tomo_bp3d_fista_momentum (no proximal operator between gradient step and momentum):
 *   X = P+(X_t - l_inv*A_s^T res);  X_t <- X + beta*(X - X_old);   methodsIR_CuPy.py:463-475
 *   on entry xold_x_dev holds X_old, on exit X;  xt_dev holds X_t on entry and the new X_t on exit. */
int tomo_bp3d_fista_momentum(tomo_ctx *ctx, int subset, const float *res_dev, float *xt_dev,
                             float *xold_x_dev, float l_inv, float beta, int nonneg, void *stream);
/* tomo_bp3d_admm:  g = A_s^T res;  z <- z - tau*(g + rho*(z - x + u));  optional max(.,0);
 *   if relax_on:  z <- (1-alpha)*z_start + alpha*z;   zu_out = z + u     methodsIR_CuPy.py:545-557
 *   (z_old of the reference equals z at the start of the sub-iteration, :555).
 *   one_minus_alpha / alpha are passed pre-rounded to float32 by the caller. */
int tomo_bp3d_admm(tomo_ctx *ctx, int subset, const float *res_dev, float *z_dev, const float *x_dev,
                   const float *u_dev, float *zu_out_dev, float tau, float rho, int relax_on,
                   float one_minus_alpha, float alpha, int nonneg, void *stream);

/* ---------------------------------------------------------------- matched back projector: the exact transpose of tomo_fp3d
 * tomo_bp3d is ASTRA's voxel-driven bilinear back projector, which is NOT the transpose of the ray-driven Joseph forward
 * projector (<Ax, y> and <x, By> differ by ~1e-1 relative on white noise).  The four entry points below
 * apply A^T itself.  No reference counterpart: parity is formula-level, UNPINNED (tests/_matched_bp_oracle.py restates it).
 * Derivation: in tomo_fp3d, voxel iy of column ix receives the tent weight max(0, 1 - |f_y - iy|) / |sin| from detector pixel
 * iu (x-stepping angle); f_y is affine in iu with slope 1/sin and equals iy exactly at iu* = f, the detector coordinate
 * tomo_bp3d computes for the voxel.  The tent has half-width |sin| <= 1 detector pixels, so it covers only i0 = floor(f) and
 * i0 + 1: the SAME two taps, other weights.  With q = tomo_angle_t::scale (y-stepping: the same with cos; equal at the tie):
 *     xw = (float)ix - half_n;  yw = (float)iy - half_n;                 half_n = 0.5f*n - 0.5f
 *     f  = fmaf(xw, cs, fmaf(yw, sn, half_u - cor));                     half_u = 0.5f*nu - 0.5f
 *     fl = floorf(f);  w = f - fl;  i0 = (int)fl;  s0 = sino[iz][a][i0], s1 = sino[iz][a][i0 + 1]   (0 outside 0 .. nu-1)
 *     w0 = max(1.0f - w*q, 0.0f) * q;   w1 = max(1.0f - (1.0f - w)*q, 0.0f) * q       (one float32 rounding per operation)
 *     acc = fmaf(w0, s0, acc);  acc = fmaf(w1, s1, acc)                  (angles ascending, tap 0 then tap 1)
 * (tomo_bp3d: w0 = 1 - w, w1 = w.)  All four take the PLANAR [nz][subset_size][nu] array and return TOMO_E_INVALID on a
 * context created with TOMO_FLAG_LERP8 (no transpose of the quantised weights is defined) or set to TOMO_RESIDUAL_ZQUAD.
 * A vertical CoR component needs nothing new: R(-shift) in front, as for tomo_bp3d. */
/* tomo_bp3d_matched: vol = A_s^T sino with the transposed Joseph weights w0, w1 derived above (vol fully overwritten). */
int tomo_bp3d_matched(tomo_ctx *ctx, int subset, const float *sino_dev, float *vol_dev, void *stream);
/* tomo_bp3d_matched_fista: tomo_bp3d_fista (arguments, aliasing, epilogue roundings) with the gradient A_s^T res formed by
 *   the transposed Joseph weights w0, w1 derived above instead of (1 - w, w). */
int tomo_bp3d_matched_fista(tomo_ctx *ctx, int subset, const float *res_dev, const float *xt_dev,
                            float *xout_dev, float l_inv, int nonneg, void *stream);
/* tomo_bp3d_matched_fista_momentum: tomo_bp3d_fista_momentum (arguments, aliasing, epilogue roundings) with the gradient
 *   formed by the transposed Joseph weights w0, w1 derived above. */
int tomo_bp3d_matched_fista_momentum(tomo_ctx *ctx, int subset, const float *res_dev, float *xt_dev,
                                     float *xold_x_dev, float l_inv, float beta, int nonneg, void *stream);
/* tomo_bp3d_matched_admm: tomo_bp3d_admm (arguments, aliasing, epilogue roundings) with g = A_s^T res formed by the
 *   transposed Joseph weights w0, w1 derived above. */
int tomo_bp3d_matched_admm(tomo_ctx *ctx, int subset, const float *res_dev, float *z_dev, const float *x_dev,
                           const float *u_dev, float *zu_out_dev, float tau, float rho, int relax_on,
                           float one_minus_alpha, float alpha, int nonneg, void *stream);

/* Private layout of the residual BETWEEN tomo_fp3d_residual and its consumer tomo_bp3d_fista / _fista_momentum / _admm on
 * the same context (round 5).  The reference materialises the residual as a [detY, angles, detX] CuPy array between
 * grad_data_term's forward and back projection (data_fidelities.py:28-40); nobody else reads it on the plain LS / PWLS /
 * KL path, so producer and consumer may agree on the layout the back projector stages fastest:
 *   TOMO_RESIDUAL_PLANAR (default): res_dev is [nz][subset_size][nu], what every entry point documents.
 *   TOMO_RESIDUAL_ZQUAD           : res_dev is [ceil(nz/4)][subset_size][nu][4] -- the four slices of a quad interleaved
 *       (slices >= nz read as 0).  The forward projector's workgroup holds exactly these four values per (angle, pixel)
 *       and stores them as ONE 16-byte word; the back projector stages one 16-byte load per (angle, quad, sample) where
 *       the planar layout costs four dword gathers from rows nz * subset_size * nu floats apart.  Same arithmetic, bit
 *       for bit.  res_dev must be 16-byte aligned and hold tomo_ctx_residual_elems(ctx, subset) floats.
 * Only the three fused epilogue entry points and tomo_fp3d_residual follow the context's setting; tomo_fp3d / tomo_bp3d
 * always take the planar layout, and tomo_fp3d_residual_ring (whose residual is read by tomo_ring_gh_reduce) refuses to
 * run while ZQUAD is set. */
enum { TOMO_RESIDUAL_PLANAR = 0, TOMO_RESIDUAL_ZQUAD = 1 };
int tomo_ctx_set_residual_layout(tomo_ctx *ctx, int layout);
int tomo_ctx_residual_layout(const tomo_ctx *ctx);
size_t tomo_ctx_residual_elems(const tomo_ctx *ctx, int subset);

/* Private layout of X_t inside the FISTA loop with a proximal step (round 7).  X_t has ONE producer there, the momentum
 * (tomo_momentum_transposed, which already writes it twice: as is and in-plane transposed), and TWO consumers:
 * tomo_fp3d_residual and the gradient-step epilogue of tomo_bp3d_fista.  The reference holds it as a [Z, Y, X] CuPy array
 * (methodsIR_CuPy.py:447-475) that nothing else reads, so the three may agree on the layout the forward projector stages
 * fastest:
 *   TOMO_VOLUME_PLANAR (default): [nz][n][n], what every entry point documents.
 *   TOMO_VOLUME_ZQUAD           : "volume zquad", [ceil(nz/4)][n][n][4] float32 -- the four slices of a quad interleaved per
 *       voxel, slices >= nz of the last quad are zeros.  The forward projector's whole-row form stages one 16-byte word per
 *       (row, column) straight into LDS (`buffer_load_dwordx4 ... lds`) where the planar layout costs four dword gathers, four
 *       prefetch registers and a ds_write_b128; the back projector reads its eight words per thread before its LDS hand-over.
 *       Same arithmetic, bit for bit.  The array must be 16-byte aligned and hold tomo_ctx_volume_elems(ctx) floats; n % 4 == 0.
 * While ZQUAD is set: tomo_momentum_transposed writes xt_dev (and the transposed token) in that layout from PLANAR x_dev /
 * xold_dev; tomo_fp3d_residual[_robust] reads vol_dev and tomo_bp3d_fista reads xt_dev in it (xout_dev stays planar).
 * tomo_volume_to_zquad converts a planar volume into the same pair (X_t = x0, once per FISTA call).  A quad-interleaved
 * volume can only be forward projected as the very next call after its producer on the same stream -- the transposed twin is
 * the one-shot token below, and nothing re-creates it -- and only where tomo_ctx_volume_zquad_ok(ctx, subset) returned 1:
 * every launch of the subset takes the whole-row double-buffered form (docs/kernels/fp.md), the back projector's brick
 * kernel serves it, and tomo_set_variant("fp", 5) -- the A/B switch of both flavours that keeps a driver on the planar
 * volume -- is not in force.  Anything else is TOMO_E_INVALID, never a quiet conversion.  tomo_fp3d, tomo_bp3d,
 * tomo_fp3d_residual_ring, tomo_bp3d_fista_momentum, tomo_bp3d_admm and the matched back projector take planar volumes
 * only (tomo_fp3d_residual_ring, tomo_bp3d_fista_momentum and tomo_bp3d_admm refuse to run while ZQUAD is set).  These five entry points joined version 10 without a raise, like
 * the ones listed at TOMO_ABI_VERSION: the tests pin the number, _lib.py binds every symbol by name. */
enum { TOMO_VOLUME_PLANAR = 0, TOMO_VOLUME_ZQUAD = 1 };
int tomo_ctx_set_volume_layout(tomo_ctx *ctx, int layout);
int tomo_ctx_volume_layout(const tomo_ctx *ctx);
size_t tomo_ctx_volume_elems(const tomo_ctx *ctx);
int tomo_ctx_volume_zquad_ok(const tomo_ctx *ctx, int subset);
int tomo_volume_to_zquad(tomo_ctx *ctx, const float *x_dev, float *xq_dev, void *stream);

/* ---------------------------------------------------------------- element-wise glue
 * tomo_momentum : x_t = x + beta*(x - x_old)                         methodsIR_CuPy.py:475
 * tomo_admm_dual: u  += z - x                                        methodsIR_CuPy.py:566
 * tomo_axpby    : y   = a*x + b*y   (Landweber / SIRT / CGLS updates, methodsIR_CuPy.py:165,222,285-295)
 * tomo_scale    : y   = a*x                                          methodsIR_CuPy.py:337
 * tomo_clamp_min: x   = max(x, lo)                                   methodsIR_CuPy.py:468,549
 * tomo_mul      : y   = x*y ;  tomo_recip_safe: y = 1/x with nan/inf -> 1 (SIRT, :206-214)
 * tomo_norm2    : sqrt(sum x^2) -> host (cp.linalg.norm,            methodsIR_CuPy.py:336,349)
 * tomo_dot      : sum x*y -> host (cp.inner, :272,284,292);  tomo_max: max -> host (:395)
 * tomo_pwls_weights: w = max(b,1e-6) / max(max(b,1e-6))              methodsIR_CuPy.py:392-395 */
int tomo_momentum(const float *x_dev, const float *xold_dev, float *xt_dev, float beta, size_t count, void *stream);
/* the same update for a context's volume [nz][n][n] that also leaves the in-plane transposed X_t in the context: the NEXT
 * tomo_fp3d* call on xt_dev (and only that one) skips its own transpose pass.  Same value as tomo_momentum, bit for bit. */
int tomo_momentum_transposed(tomo_ctx *ctx, const float *x_dev, const float *xold_dev, float *xt_dev, float beta,
                             void *stream);
/* The transposed copy is a one-shot token keyed on (xt_dev, stream): ANY following tomo_fp3d* call on the context spends
 * it, whether it can use it or not.  tomo_ctx_invalidate drops it explicitly -- call it when the volume behind xt_dev may
 * be rewritten or freed before the next forward projection (RecToolsIRCuPy.FISTA does at entry and exit, so a buffer the
 * allocator hands out again at the same address can never meet a stale copy; methodsIR_CuPy.py:447-475 has no
 * counterpart: ASTRA re-uploads the volume on every call, astra_base.py:560-606). */
int tomo_ctx_invalidate(tomo_ctx *ctx);
int tomo_admm_dual(float *u_dev, const float *z_dev, const float *x_dev, size_t count, void *stream);
int tomo_axpby(float a, const float *x_dev, float b, float *y_dev, size_t count, void *stream);
int tomo_scale(float a, const float *x_dev, float *y_dev, size_t count, void *stream);
int tomo_clamp_min(float *x_dev, float lo, size_t count, void *stream);
int tomo_mul(const float *x_dev, float *y_dev, size_t count, void *stream);
int tomo_recip_safe(const float *x_dev, float *y_dev, size_t count, void *stream);
int tomo_fill(float *x_dev, float value, size_t count, void *stream);
int tomo_norm2(const float *x_dev, size_t count, double *out_host, void *stream);
int tomo_dot(const float *x_dev, const float *y_dev, size_t count, double *out_host, void *stream);
int tomo_max(const float *x_dev, size_t count, float *out_host, void *stream);
/* Relative change between two iterates, the quantity the tolerance keys are compared with (below, "early stopping"):
 * out_host[0] = sum (x - ref)^2, out_host[1] = sum x^2, both accumulated in double from the float32 values, in ONE streaming
 * pass that also writes keep[i] = x[i] when keep_dev is given (NULL: no snapshot; keep_dev == ref_dev: "compare with the
 * snapshot and refresh it", 12 B per voxel and one launch instead of a reduction plus a copy).  Deterministic: fixed grid,
 * per-block double partials finished on the host in block order, no atomics -- the same input gives the same bits on every
 * call.  16-byte accesses when the arrays reach a 16-byte boundary after the same number of elements (scalar head / tail),
 * dword accesses otherwise.  count = 0 -> (0, 0).  Synchronises the stream (the pair is returned to the host). */
int tomo_rel_change(const float *x_dev, const float *ref_dev, float *keep_dev, size_t count, double out_host[2], void *stream);
int tomo_pwls_weights(const float *b_dev, float *w_dev, size_t count, void *stream);
/* z-slab form of the same: the caller max-all-reduces tomo_pwls_max over the slabs and passes the result on */
int tomo_pwls_max(const float *b_dev, size_t count, float *out_host, void *stream);
int tomo_pwls_weights_scaled(const float *b_dev, float *w_dev, size_t count, float wmax, void *stream);
/* diagnostics: nin-read / nout-write streaming kernel (vec = 4: float4 accesses, 1: dword) used to calibrate the
 * achievable HBM rate for a kernel's read/write mix (tools/archive/probes/stream_probe.py) */
int tomo_diag_stream(const float *const *in_dev, int nin, float *const *out_dev, int nout, size_t count,
                     int vec, int grid, void *stream);

/* ---------------------------------------------------------------- pre/post glue
 * tomo_pad_edge   : edge-pad detX by `pad` both sides, [nz][na][nu0] -> [nz][na][nu0+2pad]
 *                   (_apply_horiz_detector_padding, supp/suppTools.py:425-459)
 * tomo_crop_center: centre-crop y,x  [nz][n][n] -> [nz][m][m]  (perform_recon_crop, suppTools.py:399-422)
 * tomo_circ_mask  : in-place disc mask of apply_circular_mask (suppTools.py:364-396)
 * tomo_permute3   : out[i][j][k] = in laid out with strides (s0,s1,s2) -- materialises the axis swap of
 *                   _data_dims_swapper (supp/funcs.py:190-206) as a contiguous array */
int tomo_pad_edge(const float *in_dev, float *out_dev, int rows, int nu0, int pad, void *stream);
int tomo_crop_center(const float *in_dev, float *out_dev, int nz, int n, int m, void *stream);
int tomo_circ_mask(float *vol_dev, int nz, int n, double radius, void *stream);
int tomo_permute3(const float *in_dev, float *out_dev, int d0, int d1, int d2,
                  int64_t s0, int64_t s1, int64_t s2, void *stream);

/* ---------------------------------------------------------------- TV proximal operators
 * tomo_pdtv replaces PD_TV_cupy's device work (regularisersCuPy.py:220-296) and the 16 kernels
 *   primal_dual_for_total_variation_{2D,3D}_{float,half}[_nonneg][_methodTV]
 *   (cuda_kernels/primal_dual_for_total_variation.cu:263-301,454-492).
 *   dims: dx fastest.  nd = 2 -> [dy][dx] (dz ignored), nd = 3 -> [dz][dy][dx].
 *   sigma,tau,lt,theta are the float32 scalars of regularisersCuPy.py:215-218 (computed by the caller).
 *   half != 0 stores the dual fields as IEEE binary16.  out_dev receives U_arrays[iters % 2].
 * tomo_roftv replaces ROF_TV_cupy's device work (regularisersCuPy.py:78-167) and
 *   divergence_kernel_* / TV_kernel_* (cuda_kernels/rudin_osher_fatemi_total_variation.cu:106-148,203-248);
 *   the two kernels are fused (the D fields never reach HBM); half != 0 rounds D through binary16.
 * `device` selects the GPU (gpu_id argument of the reference functions). */
int tomo_pdtv(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
              float sigma, float tau, float lt, float theta, int iters, int methodTV, int nonneg,
              int half, void *stream);
int tomo_roftv(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
               float lambda, float tau, int iters, int half, void *stream);
/* Early stopping (the `tolerance` keys of the dictionaries; no implementation in this reference version -- the rule is this
 * project's, formula-level parity, unpinned).  For iterates v_0 = input, v_n = what the operator returns after n iterations:
 *     d_n = sqrt( sum (v_n - v_{n-6})^2 / sum v_n^2 )     (tomo_rel_change; 0 when the numerator is 0, +inf when only the
 *                                                            denominator is)
 * evaluated after iteration n when n is a multiple of 6 and at least 3 of the requested iterations remain; the loop stops
 * after iterate n when tol > 0 and d_n < tol, and out_dev then holds exactly what iters = n without a tolerance returns.
 * tol is a double so that the threshold compared with is the one the user wrote; negative / non-finite: TOMO_E_INVALID.
 * *iters_done receives n (iters if the rule was never met), *last_rel_change the last d evaluated (NaN if none was); either
 * may be NULL.  tol = 0 is tomo_pdtv / tomo_roftv launch for launch (one shared loop).  With tol > 0 every check is one
 * tomo_rel_change pass and one stream synchronisation, and the iterate of six iterations ago lives in a block of its own
 * (one float volume, plain allocation per (device, stream), freed by tomo_release_scratch) BESIDE the arena that
 * tomo_pdtv_scratch_bytes / tomo_roftv_scratch_bytes describe, whose size and placement do not change. */
int tomo_pdtv_tol(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                  float sigma, float tau, float lt, float theta, int iters, int methodTV, int nonneg,
                  int half, double tol, int *iters_done, double *last_rel_change, void *stream);
int tomo_roftv_tol(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                   float lambda, float tau, int iters, int half, double tol, int *iters_done,
                   double *last_rel_change, void *stream);
/* Slice-wise PD_TV / ROF_TV (no reference counterpart; docs/kernels/slicewise.md): in_dev is a stack [nslices][dy][dx] and
 * every (y, x) slice receives exactly what tomo_pdtv / tomo_roftv with nd = 2 return for it -- the same iteration and the
 * same roundings (PD_TV variants 0 and 22, ROF_TV variant 0), nothing couples the slices -- with all slices in one launch
 * (PD_TV: up to three iterations per launch; ROF_TV: one).  Scalars, flags, checks and error texts as for tomo_pdtv /
 * tomo_roftv (ROF_TV needs dx, dy >= 2); iters = 0 copies the input; tomo_roftv_slices iterates in out_dev, which must not
 * alias in_dev.  tol, iters_done, last_rel_change: the rule of tomo_pdtv_tol with ONE decision over the whole stack, so
 * every slice runs the same number of iterations and a stopped run leaves exactly what iters = n returns.  Work arrays in
 * the placed TV arena: tomo_pdtv_slices_scratch_bytes (U ping-pong and two dual fields in and out, float32 or binary16),
 * tomo_roftv_slices_scratch_bytes (the one ping-pong partner of out_dev). */
int tomo_pdtv_slices(int device, const float *in_dev, float *out_dev, int dx, int dy, int nslices, float sigma,
                     float tau, float lt, float theta, int iters, int methodTV, int nonneg, int half, double tol,
                     int *iters_done, double *last_rel_change, void *stream);
int tomo_roftv_slices(int device, const float *in_dev, float *out_dev, int dx, int dy, int nslices, float lambda,
                      float tau, int iters, int half, double tol, int *iters_done, double *last_rel_change,
                      void *stream);
size_t tomo_pdtv_slices_scratch_bytes(int dx, int dy, int nslices, int half);
size_t tomo_roftv_slices_scratch_bytes(int dx, int dy, int nslices);
/* Second-order total generalised variation (TGV): argmin_u 1/2 |u - f|^2 + lambda min_v (alpha1 |grad u - v|_1 + alpha0 |E v|_1)
 * by Chambolle-Pock iterations.  No reference counterpart in this reference version (it took TGV from the regularisation
 * toolkit it no longer depends on; tomobar/supp/dicts.py:176-178 still names PD_LipschitzConstant "TGV specific"): the
 * algorithm is stated in docs/kernels/tgv.md and restated in numpy by tests/_tgv_oracle.py -- formula-level parity,
 * unpinned; the float32 result equals that restatement bit for bit.
 *   dims as for tomo_pdtv (a dimension of 1 is valid).  lambda, alpha1, alpha0, tau, sigma are float32 scalars computed by
 *   the caller (TGV_cupy: tau = sigma = 1 / sqrt(PD_LipschitzConstant)).  U is iterated in out_dev, which therefore must not
 *   alias in_dev (TOMO_E_INVALID, as are nd outside {2, 3}, a dimension below 1, a non-positive lambda / alpha1 / alpha0 /
 *   step size, negative iters and a negative or non-finite tol).  iters = 0 copies the input.  Two launches per iteration.
 *   tol, *iters_done, *last_rel_change: the early-stopping rule above (tol = 0: off); a stopped run leaves exactly what
 *   iters = n returns. */
int tomo_tgv(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
             float lambda, float alpha1, float alpha0, float tau, float sigma, int iters,
             double tol, int *iters_done, double *last_rel_change, void *stream);
/* The launches of PDHG (primal-dual hybrid gradient, Chambolle-Pock, on min_x F(Ax) + lambda TV(x) itself) beside the
 * forward projector and the matched back projector: RecToolsIRCuPy.PDHG runs, per iteration, tomo_fp3d on x-bar,
 * tomo_pdhg_sino_dual, tomo_bp3d_matched, tomo_pdhg_tv_dual, tomo_pdhg_primal.  No reference counterpart: the algorithm is
 * stated in docs/kernels/pdhg.md and restated in numpy by tests/_pdhg_oracle.py -- formula-level parity, unpinned; the
 * float32 results equal that restatement bit for bit.  All scalars are float32 values computed by the caller.
 *   tomo_pdhg_sino_dual: y <- prox of the conjugate of the data term, element-wise over `count` samples, in place; r = A x-bar,
 *     b = the data.  TOMO_PDHG_LS: (y + sigma (r - b)) / (1 + sigma); TOMO_PDHG_L1: the same ascent clipped to [-1, 1];
 *     TOMO_PDHG_KL: v = y + sigma r, y = 0.5 ((1 + v) - sqrt((v - 1)^2 + 4 sigma max(b, 0))).  16-byte accesses when the
 *     three arrays are 16-byte aligned, with a scalar tail.  TOMO_E_INVALID: an unknown term, a non-positive sigma, NULL,
 *     y aliasing r or b.
 *   tomo_pdhg_tv_dual: q_d <- q_d + sigma F_d(x-bar) (forward differences, 0 on the last index), then q / max(1, |q| /
 *     lambda) (methodTV 0) or the clip to [-lambda, lambda] (methodTV 1), in place.  dims as for tomo_pdtv (a dimension of
 *     1 is valid); nd = 2 ignores dz and q3_dev.
 *   tomo_pdhg_primal: x' = x - tau (g - div q), div q = (B_1 q1 + B_2 q2) + B_3 q3 (backward differences), clamped at 0
 *     with nonneg; x-bar <- (x' + x') - x, x <- x', in place.  q1_dev = q2_dev = q3_dev = NULL: no TV block, div q = 0.
 *   Both marches: TOMO_E_INVALID for nd outside {2, 3}, a dimension below 1, a non-positive step size or lambda, NULL or
 *     aliasing arrays.  One launch each.
 *   tomo_pdhg_scratch_bytes: 2 + nd float arrays (x-bar, g, q_1..q_nd), each rounded up to 256 bytes and followed by the
 *     69888-byte array skew -- the layout of a tomo_placed_scratch block the driver takes them from. */
enum { TOMO_PDHG_LS = 0, TOMO_PDHG_L1 = 1, TOMO_PDHG_KL = 2 };
size_t tomo_pdhg_scratch_bytes(int dx, int dy, int dz, int nd);
int tomo_pdhg_sino_dual(float *y_dev, const float *r_dev, const float *b_dev, size_t count, int fidelity, float sigma,
                        void *stream);
int tomo_pdhg_tv_dual(int device, const float *xbar_dev, float *q1_dev, float *q2_dev, float *q3_dev, int dx, int dy,
                      int dz, int nd, float sigma, float lambda, int methodTV, void *stream);
int tomo_pdhg_primal(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *q1_dev,
                     const float *q2_dev, const float *q3_dev, int dx, int dy, int dz, int nd, float tau, int nonneg,
                     void *stream);
/* PDHG with the diagonal preconditioner of Pock and Chambolle (alpha = 1; RecToolsIRCuPy.PDHG with
 * _algorithm_["PDHG_preconditioner"] = "diagonal", docs/kernels/pdhg.md): a step per sample and a step per voxel in place of
 * the two scalars.  The same kernels with one more array stream each; bit for bit tests/_pdhg_diag_oracle.py.
 *   tomo_pdhg_diag_steps: out = numer / max(in + add, 2^-10) over `count` elements, max as the comparison v < eps ? eps : v:
 *     the steps from the row sums A 1 (add = 0) or the column sums A^T 1 (add = 2 nd with TV).  out_dev == in_dev is
 *     allowed.  TOMO_E_INVALID: a non-positive numer, a negative add, NULL.
 *   tomo_pdhg_sino_dual_diag: tomo_pdhg_sino_dual with sigma_dev[i] in place of sigma (1 + sigma_i and 4 sigma_i are
 *     computed per sample); 20 B per sample.  TOMO_E_INVALID: an unknown term, NULL, y aliasing r, b or sigma.
 *   tomo_pdhg_primal_diag: tomo_pdhg_primal with tau_dev[j] in place of tau, one more plane stream (32 B per voxel with TV).
 *     TOMO_E_INVALID as for tomo_pdhg_primal; tau_dev must not be NULL nor alias x, x-bar or g.
 *   tomo_pdhg_diag_scratch_bytes: tomo_pdhg_scratch_bytes plus one more skewed array, tau, behind the others. */
size_t tomo_pdhg_diag_scratch_bytes(int dx, int dy, int dz, int nd);
int tomo_pdhg_diag_steps(float *out_dev, const float *in_dev, size_t count, float numer, float add, void *stream);
int tomo_pdhg_sino_dual_diag(float *y_dev, const float *r_dev, const float *b_dev, const float *sigma_dev, size_t count,
                             int fidelity, void *stream);
int tomo_pdhg_primal_diag(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *tau_dev,
                          const float *q1_dev, const float *q2_dev, const float *q3_dev, int dx, int dy, int dz, int nd,
                          int nonneg, void *stream);
/* PDHG with the second-order TGV term lambda min_v (alpha1 |grad x - v| + alpha0 |E v|) in its dual (RecToolsIRCuPy.PDHG with
 * _regularisation_["method"] = "PD_TGV", docs/kernels/pdhg.md): two plane marches in place of tomo_pdhg_tv_dual and
 * tomo_pdhg_primal; bit for bit tests/_pdhg_tgv_oracle.py.  The fields of the TGV block are passed as host arrays of device
 * pointers: v, v-bar and P hold nd, Q holds 3 (nd = 2: Q11, Q22, Q12) or 6 (nd = 3: Q11, Q22, Q12, Q33, Q13, Q23).
 *   tomo_pdhg_tgv_dual: P_d <- P_d + sigma_p (F_d(x-bar) - v-bar_d), then P / max(1, |P| / r1); Q <- Q + sigma_q E(v-bar)
 *     (symmetrised forward differences), then Q / max(1, |Q|_F / r0), off-diagonal components counted twice; in place,
 *     88 B per voxel in 3D.  r1 = lambda alpha1, r0 = lambda alpha0.  TOMO_E_INVALID: non-positive steps or radii, NULL, P or
 *     Q aliasing each other, x-bar or v-bar, a plane of 2^29 voxels or more.
 *   tomo_pdhg_tgv_primal: x' = x - tau_x (g - div P), clamped at 0 with nonneg; x-bar <- (x' + x') - x, x <- x';
 *     v'_d = v_d + tau_v (P_d + B_d(Q_dd) + sum_{e != d} B_e(Q_de)), v-bar_d <- (v'_d + v'_d) - v_d, v_d <- v'_d (never
 *     clamped); in place, 88 B per voxel in 3D.  TOMO_E_INVALID: non-positive steps, NULL, any two arrays aliasing, the plane
 *     limit.
 *   tomo_pdhg_tgv_primal_diag: the same with tau_dev[j] in place of tau_x, one more plane stream (92 B).
 *   tomo_pdhg_tgv_scratch_bytes: 17 (nd = 3) or 11 (nd = 2) float arrays -- x-bar, g, P, Q, v, v-bar --, each rounded up to
 *     256 bytes and followed by the skew of the TV arena; tomo_pdhg_tgv_diag_scratch_bytes: one more, tau, behind them. */
size_t tomo_pdhg_tgv_scratch_bytes(int dx, int dy, int dz, int nd);
size_t tomo_pdhg_tgv_diag_scratch_bytes(int dx, int dy, int dz, int nd);
int tomo_pdhg_tgv_dual(int device, const float *xbar_dev, const float *const *vbar_dev, float *const *p_dev, float *const *q_dev,
                       int dx, int dy, int dz, int nd, float sigma_p, float sigma_q, float r1, float r0, void *stream);
int tomo_pdhg_tgv_primal(int device, float *x_dev, float *xbar_dev, const float *g_dev, float *const *v_dev,
                         float *const *vbar_dev, const float *const *p_dev, const float *const *q_dev, int dx, int dy, int dz,
                         int nd, float tau_x, float tau_v, int nonneg, void *stream);
int tomo_pdhg_tgv_primal_diag(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *tau_dev,
                              float *const *v_dev, float *const *vbar_dev, const float *const *p_dev, const float *const *q_dev,
                              int dx, int dy, int dz, int nd, float tau_v, int nonneg, void *stream);
/* PDHG with a stripe variable for ring artefacts (RecToolsIRCuPy.PDHG with _data_["stripe_lambda"]; docs/kernels/pdhg.md,
 * "The stripe variable"): min_{x, s} F(A x + S s; b) + lambda R(x) + mu |s|_1, s[z][u] one offset per detector pixel,
 * (S s)[z][a][u] = s[z][u].  The sinogram is [nz][na][nu], u fastest; the angles are cut into n_seg = ceil(na /
 * TOMO_PDHG_STRIPE_SEG) segments of TOMO_PDHG_STRIPE_SEG rows, so that the sum of y over the angles is deterministic and
 * still parallel along them.  No reference counterpart: tests/_pdhg_stripe_oracle.py restates both launches in numpy and
 * they equal its float32 form bit for bit (one rounding per operation, no FMA contraction).
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
#define TOMO_PDHG_STRIPE_SEG 64
int tomo_pdhg_sino_dual_stripe(float *y_dev, const float *r_dev, const float *b_dev, const float *sigma_dev,
                               const float *sbar_dev, float *part_dev, int nz, int na, int nu, int fidelity, float sigma,
                               void *stream);
int tomo_pdhg_stripe_update(float *s_dev, float *sbar_dev, const float *part_dev, int nz, int na, int nu, float tau_s,
                            float theta, void *stream);
/* The launches of SPDHG (stochastic PDHG over ordered subsets: one block update touches one subset of angles or the TV
 * block) beside the per-subset forward projector and the subset form of the matched back projector: a subset update of
 * RecToolsIRCuPy.SPDHG runs tomo_fp3d on x, tomo_spdhg_sino_dual, tomo_bp3d_matched, tomo_spdhg_primal; a TV update runs
 * tomo_spdhg_tv_dual, tomo_spdhg_tv_primal.  No reference counterpart: the algorithm is stated in docs/kernels/spdhg.md and
 * restated in numpy by tests/_spdhg_oracle.py -- formula-level parity, unpinned; the float32 results equal that restatement
 * bit for bit.  All scalars are float32 values computed by the caller; `w` is 1 / the block's probability.
 *   tomo_spdhg_sino_dual: v = the update of tomo_pdhg_sino_dual (same `fidelity`) on (y, r, b) over `count` samples;
 *     r <- v - y (the change the back projector takes), y <- v, both in place.  16-byte accesses when the three arrays are
 *     16-byte aligned, with a scalar tail.  TOMO_E_INVALID: an unknown term, a non-positive sigma, NULL, aliasing arrays.
 *   tomo_spdhg_primal: z' = z + delta, zb = z' + w delta, x' = x - tau zb, clamped at 0 with nonneg; x <- x', z <- z', in
 *     place over `count` voxels (delta = A_j^T of the change).  The same two access forms.  TOMO_E_INVALID: a non-positive
 *     tau or w, NULL, aliasing arrays.
 *   tomo_spdhg_tv_dual: p_d = the update of tomo_pdhg_tv_dual on (x, q) (methodTV 0 / 1, radius lambda); e_d <- p_d - q_d,
 *     q_d <- p_d.  dims as for tomo_pdtv (a dimension of 1 is valid); nd = 2 ignores dz, q3_dev and e3_dev.
 *   tomo_spdhg_tv_primal: div = (B_1 e1 + B_2 e2) + B_3 e3 (backward differences); z' = z - div, zb = z' - w div,
 *     x' = x - tau zb, clamped at 0 with nonneg; x <- x', z <- z', in place.
 *   Both marches: TOMO_E_INVALID for nd outside {2, 3}, a dimension below 1, a non-positive step size, weight or lambda,
 *     NULL or aliasing arrays.  One launch each.
 *   tomo_spdhg_scratch_bytes: 2 + 2 nd float arrays (z, delta, q_1..q_nd, e_1..e_nd), each rounded up to 256 bytes and
 *     followed by the 69888-byte array skew -- the layout of a tomo_placed_scratch block the driver takes them from. */
size_t tomo_spdhg_scratch_bytes(int dx, int dy, int dz, int nd);
int tomo_spdhg_sino_dual(float *y_dev, float *r_dev, const float *b_dev, size_t count, int fidelity, float sigma,
                         void *stream);
int tomo_spdhg_primal(float *x_dev, float *z_dev, const float *delta_dev, size_t count, float tau, float w, int nonneg,
                      void *stream);
int tomo_spdhg_tv_dual(int device, const float *x_dev, float *q1_dev, float *q2_dev, float *q3_dev, float *e1_dev,
                       float *e2_dev, float *e3_dev, int dx, int dy, int dz, int nd, float sigma, float lambda, int methodTV,
                       void *stream);
int tomo_spdhg_tv_primal(int device, float *x_dev, float *z_dev, const float *e1_dev, const float *e2_dev,
                         const float *e3_dev, int dx, int dy, int dz, int nd, float tau, float w, int nonneg, void *stream);
/* Nonlinear diffusion (NDF) by explicit time marching: U^0 = in, n times
 *     U' = U + tau (lambda S - (U - in)),   S = sum over the axes of g(U[i + e] - U[i]) + g(U[i - e] - U[i]),
 * with zero flux through the faces of the volume and the flux g chosen by `penalty`:
 *     TOMO_NDF_HUBER  g(t) = t / sigma where |t| <= sigma, else sign(t)                    (behaves like TV)
 *     TOMO_NDF_PM     g(t) = t / (1 + (t / sigma)^2)                                       (Perona-Malik: sharpens edges)
 *     TOMO_NDF_TUKEY  g(t) = t (1 - (t / sigma)^2)^2 where |t| <= sigma, else 0            (edges above sigma untouched)
 * The reference's dicts_check names NDF among the users of time_marching_step (tomobar/supp/dicts.py:173) but nothing in
 * its tree implements it: the algorithm, with its order of operations, is stated in docs/kernels/ndf.md and restated in
 * numpy by tests/_ndf_oracle.py -- formula-level parity, unpinned; the float32 result equals that restatement bit for bit.
 *   dims as for tomo_pdtv (a dimension of 1 is valid).  lambda (regul_param), sigma (edge_threshold) and tau
 *   (time_marching_step) are float32 scalars.  The iterations ping-pong between out_dev and one work array of the TV arena,
 *   so out_dev must not alias in_dev (TOMO_E_INVALID, as are nd outside {2, 3}, a dimension below 1, a non-positive lambda /
 *   sigma / tau, a penalty outside {0, 1, 2}, negative iters and a negative or non-finite tol); in_dev is never written.
 *   iters = 0 copies the input.  One launch per iteration, 12 B per voxel.
 *   tol, *iters_done, *last_rel_change: the early-stopping rule above (tol = 0: off); a stopped run leaves exactly what
 *   iters = n returns. */
enum { TOMO_NDF_HUBER = 0, TOMO_NDF_PM = 1, TOMO_NDF_TUKEY = 2 };
int tomo_ndf(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
             float lambda, float sigma, float tau, int penalty, int iters,
             double tol, int *iters_done, double *last_rel_change, void *stream);
/* Diff4th: anisotropic fourth-order diffusion (Hajiaboli), explicit in time: U^0 = in, n times
 *     W  = cw^2 eta + cw (L - eta),   cw = 1 / (1 + G / sigma^2),
 *     U' = U - tau (lambda B + (U - in)),   B = sum over the axes of W[i + e] + W[i - e] - 2 W[i],
 * with G the squared central-difference gradient of U, L its Laplacian and eta = Q / G its second derivative along the
 * gradient (0 where G = 0); every neighbour index is clamped into the volume.  The reference's dicts_check names Diff4th
 * among the users of time_marching_step (tomobar/supp/dicts.py:173) but nothing in its tree implements it: the algorithm,
 * with its order of operations, is stated in docs/kernels/diff4th.md and restated in numpy by tests/_diff4th_oracle.py --
 * formula-level parity, unpinned; the float32 result equals that restatement bit for bit.
 *   dims as for tomo_pdtv (a dimension of 1 is valid).  lambda (regul_param), sigma (edge_threshold) and tau
 *   (time_marching_step) are float32 scalars; the scheme is explicit and stable for tau (1 + 16 nd^2 lambda) <~ 1, which
 *   is not checked.  The iterations ping-pong between out_dev and one work array of the TV arena, so out_dev must not alias
 *   in_dev (TOMO_E_INVALID, as are nd outside {2, 3}, a dimension below 1, a non-positive lambda / sigma / tau, negative
 *   iters and a negative or non-finite tol); in_dev is never written.  iters = 0 copies the input.  One launch per
 *   iteration (both stages fused, W stays in registers), 12 B per voxel.
 *   tol, *iters_done, *last_rel_change: the early-stopping rule above (tol = 0: off); a stopped run leaves exactly what
 *   iters = n returns. */
int tomo_diff4th(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                 float lambda, float sigma, float tau, int iters,
                 double tol, int *iters_done, double *last_rel_change, void *stream);
/* LLT_ROF: ROF total variation plus the fourth-order Lysaker-Lundervold-Tai term, explicit in time: U^0 = in, n times
 *     R_d = a_d / sqrt(sum a_e^2 + eps),   E_d = h_d / (|h_d| + eps),   eps = 1e-8,
 *     U' = U - tau ((lambda_llt B - lambda_rof V) + (U - in)),
 * with a_d the forward and h_d the second difference of U along axis d (every neighbour index clamped into the volume),
 * V = sum over the axes of R_d[i] - R_d[i - e_d] (zero for the missing backward neighbour: the divergence) and
 * B = sum over the axes of E_d[i + e_d] + E_d[i - e_d] - 2 E_d[i] (the index of E_d clamped).  The reference's dicts_check
 * names LLT_ROF among the users of time_marching_step (tomobar/supp/dicts.py:173) but nothing in its tree implements it:
 * the algorithm, with its order of operations, is stated in docs/kernels/llt_rof.md and restated in numpy by
 * tests/_llt_rof_oracle.py -- formula-level parity, unpinned; the float32 result equals that restatement bit for bit.
 *   dims as for tomo_pdtv (a dimension of 1 is valid).  lambda_rof (regul_param), lambda_llt (regul_param2) and tau
 *   (time_marching_step) are float32 scalars; the fluxes are bounded by 1, so no step bound is checked.  The iterations
 *   ping-pong between out_dev and one work array of the TV arena, so out_dev must not alias in_dev (TOMO_E_INVALID, as are
 *   nd outside {2, 3}, a dimension below 1, a non-positive lambda_rof / lambda_llt / tau, negative iters and a negative or
 *   non-finite tol); in_dev is never written.  iters = 0 copies the input.  One launch per iteration (both stages fused,
 *   the six flux fields stay in registers), 12 B per voxel.
 *   tol, *iters_done, *last_rel_change: the early-stopping rule above (tol = 0: off); a stopped run leaves exactly what
 *   iters = n returns. */
int tomo_llt_rof(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                 float lambda_rof, float lambda_llt, float tau, int iters,
                 double tol, int *iters_done, double *last_rel_change, void *stream);
/* Wavelet shrinkage W_t, the `_WAVELETS` suffix of a regularisation method: every (y, x) slice (nd = 3: dz independent
 * slices, nd = 2: one) goes through three levels of the 2D orthonormal Daubechies-5 transform in periodization mode (an
 * odd line is extended by a copy of its last sample; x is filtered first, then y), every detail coefficient d of every
 * level becomes copysign(max(|d| - threshold, 0), d), and the inverse transform follows.  The reference's tutorials use
 * "PD_TV_WAVELETS" (docs/source/tutorials/regul_iter_recon.rst:113) but nothing in its tree implements the step (it lived
 * in the removed RecToolsIR class, on the CUDA-only pypwt package): the algorithm, with its order of operations, is stated
 * in docs/kernels/wavelets.md and restated in numpy by tests/_wavelet_oracle.py -- formula-level parity, unpinned; the
 * float32 result equals that restatement bit for bit.
 *   dims as for tomo_pdtv (a dimension of 1 is valid).  threshold >= 0 (0: the identity up to rounding).
 *   The pyramid of a slice holds, for level l = 1, 2, 3 in this order (n_0 = n, n_l = ceil(n_{l-1} / 2)), the bands LL, LH,
 *   HL, HH of dy_l x dx_l floats each (first letter: the x filter, second: the y filter); the pyramids of the slices follow
 *   each other.  tomo_wavelet_scratch_bytes is the size of all of them (4 sum_l dy_l dx_l floats per slice, about 1.33
 *   volumes; 0 for invalid dims).  LL_1 and LL_2 are work space: the forward pass leaves the approximations there, the
 *   inverse pass overwrites them with its own.
 *   tomo_wavelet_shrink: in_dev -> out_dev through a pyramid in the TV scratch arena of (device, stream), six launches (one
 *   forward and one inverse per level: tiles staged in LDS with their circular apron, the threshold applied as the bands
 *   are written).  mix_dev (or NULL): an array laid out like out_dev; the last launch then stores (mix + W_t(in)) * 0.5f,
 *   reading mix at the index it writes, so mix_dev may be out_dev itself.  in_dev may alias out_dev.
 *   tomo_wavelet_forward writes the thresholded pyramid of in_dev into pyramid_dev (the caller's, of
 *   tomo_wavelet_scratch_bytes); tomo_wavelet_inverse reads one (and overwrites its LL_1 and LL_2) into out_dev.
 *   TOMO_E_INVALID: a negative (or NaN) threshold, nd outside {2, 3}, a dimension < 1, a NULL array, a negative device. */
size_t tomo_wavelet_scratch_bytes(int dx, int dy, int dz, int nd);
int tomo_wavelet_shrink(int device, const float *in_dev, float *out_dev, const float *mix_dev, int dx, int dy, int dz,
                        int nd, float threshold, void *stream);
int tomo_wavelet_forward(int device, const float *in_dev, float *pyramid_dev, int dx, int dy, int dz, int nd,
                         float threshold, void *stream);
int tomo_wavelet_inverse(int device, float *pyramid_dev, float *out_dev, const float *mix_dev, int dx, int dy, int dz,
                         int nd, void *stream);
/* Non-local total variation (NLTV): PatchSelect builds the neighbour tables, the NLTV iteration uses them.  The
 * reference's legacy demo (Demos/methods_IR_legacy/DemoFISTA_NLTV_2D.py) passes such tables under NLTV_H_i, NLTV_H_j and
 * NLTV_Weights, but both halves lived in the regularisation toolkit it no longer depends on: the algorithm, with its order
 * of operations and its own exponential, is stated in docs/kernels/nltv.md and restated in numpy by tests/_nltv_oracle.py
 * -- formula-level parity, unpinned; the float32 results (indices included) equal that restatement bit for bit.
 *   dims as for tomo_pdtv (a dimension of 1 is valid), except that dx and dy may not exceed 65535 (the index tables are
 *   16-bit).  nd = 3 is a stack of dz independent (y, x) slices: search, patches and iteration never leave a slice.
 *   The tables are laid out [neighbours][dz][dy][dx]: hi_dev the x index and hj_dev the y index of the k-th neighbour of
 *   every pixel (uint16), w_dev its weight (float32) -- 8 * neighbours bytes per voxel in all.
 *   tomo_patch_select: for every pixel the `neighbours` (1..32) offsets of [-search, search]^2 without (0, 0) (search
 *   1..15) that lie inside the slice and have the smallest patch distance d -- a separable Gaussian-weighted sum of squared
 *   differences over a (2 patch + 1)^2 patch (patch 1..4), terms outside the slice dropped --, ties to the earlier offset
 *   (row-major order), stored in ascending order of d with the weight exp(-d / h^2); a pixel with fewer candidates than
 *   `neighbours` fills the rest with its own index and the weight 0.  One launch (per 65535 slices), no scratch.
 *   tomo_nltv: u^0 = in, `iters` Jacobi iterations of
 *       u' = (f / lambda + c sum_k w_k u_k) / (1 / lambda + c sum_k w_k),   c = 2 / sqrt(sum_k w_k (u_k - u)^2 + 1e-12),
 *   with u_k = u[hj_k, hi_k] inside the pixel's slice.  Every index is clamped into the slice before use (a valid table is
 *   not changed by that; a corrupt one gives a wrong answer, never an access outside the array).  The iterations ping-pong
 *   between out_dev and one work array of the TV arena (tomo_nltv_scratch_bytes), so out_dev must not alias in_dev; in_dev
 *   and the tables are never written.  iters = 0 copies the input.  One launch per iteration, 8 * neighbours + 12 B per voxel.
 *   tol, *iters_done, *last_rel_change: the early-stopping rule above (tol = 0: off).
 *   TOMO_E_INVALID: search, patch or neighbours outside their ranges, dx or dy above 65535, a dimension < 1, nd outside
 *   {2, 3}, a NULL array, a non-positive h or lambda, negative iters, a negative or non-finite tol, out_dev == in_dev. */
size_t tomo_nltv_scratch_bytes(int dx, int dy, int dz, int nd);
int tomo_patch_select(int device, const float *in_dev, uint16_t *hi_dev, uint16_t *hj_dev, float *w_dev,
                      int dx, int dy, int dz, int nd, int search, int patch, int neighbours, float h, void *stream);
int tomo_nltv(int device, const float *in_dev, float *out_dev, const uint16_t *hi_dev, const uint16_t *hj_dev,
              const float *w_dev, int dx, int dy, int dz, int nd, int neighbours, float lambda, int iters,
              double tol, int *iters_done, double *last_rel_change, void *stream);
/* scratch bytes the TV drivers hold for a given problem (informational; a tolerance adds one float volume, see above) and
 * arena release.  tomo_tgv_scratch_bytes: 16 (nd = 3: U-bar, V, V-bar, P, six Q) or 10 (nd = 2) float arrays, each rounded
 * up to 256 bytes and followed by the 69888-byte array skew.  tomo_ndf_scratch_bytes, tomo_diff4th_scratch_bytes and
 * tomo_llt_rof_scratch_bytes: one such array (the ping-pong partner of the output array). */
size_t tomo_pdtv_scratch_bytes(int dx, int dy, int dz, int nd, int half);
size_t tomo_roftv_scratch_bytes(int dx, int dy, int dz, int nd);
size_t tomo_tgv_scratch_bytes(int dx, int dy, int dz, int nd);
size_t tomo_ndf_scratch_bytes(int dx, int dy, int dz, int nd);
size_t tomo_diff4th_scratch_bytes(int dx, int dy, int dz, int nd);
size_t tomo_llt_rof_scratch_bytes(int dx, int dy, int dz, int nd);
int tomo_release_scratch(int device);
/* Placement of the TV scratch arenas (no reference counterpart: CuPy's memory pool hands out whatever block comes next).
 * On MI355X the speed of the plane-marching TV kernels depends on where in HBM their arrays lie (PD_TV launch at 1024^3:
 * 10.1 ms with the arena in one block, 9.1-9.3 ms in another of the same process; docs/kernels/placement.md).  The TV
 * operators' own arena and the tomo_placed_scratch blocks -- nothing else: FBP spectra, Fourier and reduction scratch are
 * plain allocations -- are therefore chosen, when they are >= 1 GiB, among up to `tries` candidate allocations held at
 * once, each scored by a ~7 ms z-march probe; the search stops at the first candidate 8 % above an earlier one (the
 * "fast class"), keeps the best and frees the rest.  Default 8 tries (environment TOMO_MI355X_PLACE_TRIES, at most 10),
 * 1 = plain hipMalloc.  Bounds on what the search may hold TRANSIENTLY: the candidates together never exceed 85 % of the
 * memory that was free when the search began, and a further candidate is only taken while the device keeps 4 GiB free;
 * one search runs at a time per process, outside the lock that guards the other arenas.  A caller that shares the GPU
 * with another allocator and cannot afford the transient footprint (up to tries x arena bytes) sets tries = 1.
 * tomo_placement_last reports the most recent search of this process: returns the number of candidates scored
 * (0 = none yet), *bytes the block size, *chosen the index kept, scores_GBps[i] the probe rate of candidate i;
 * tomo_placement_last_fast: 1 if the kept block cleared the 8 % rule, 0 if the tries ran out first, -1 if none ran. */
/* Allocate (and place) the TV operators' scratch arena of this (device, stream) ahead of the first call that needs it --
 * e.g. tomo_pdtv_scratch_bytes(...) at set-up time, so that the placement search (0.1-4 s) is not part of the first
 * iteration (RecToolsIRCuPy.FISTA / ADMM / OSEM do this before their loops).  Grow-only like every arena: a later call
 * that needs more re-allocates. */
int tomo_reserve_scratch(int device, size_t bytes, void *stream);
int tomo_set_placement_tries(int tries);
int tomo_placement_tries(void);
/* A placed scratch block for callers that keep their own plane-marching work arrays (the z-slab drivers hold ghosted
 * copies of U, P1..3 and Input per rank; the reference's multi-GPU demo has cupy allocate them,
 * Demos/methods_IR_legacy/MultiGPU_demo.py:144-190): `bytes` of device memory owned by the library, one block per
 * (device, stream, slot 0..7), grow-only -- asking a slot for MORE than it holds frees the old block, so earlier pointers
 * into it die --, released by tomo_release_scratch.  Placement as above. */
int tomo_placed_scratch(int device, int slot, size_t bytes, void *stream, void **out_dev);
int tomo_placement_last(size_t *bytes, int *chosen, double *scores_GBps, int capacity);
int tomo_placement_last_fast(void);

/* Slab (multi-GPU) form of one PD-TV iteration on arrays that carry ghost planes:
 *   every array pointer addresses [has_lo + nz_local + has_hi][dy][dx]; the planes at either end are
 *   the neighbours' boundary planes (read-only).  Boundary rules (zIndex>0 / last_z of
 *   primal_dual_for_total_variation.cu:188,213) apply only where has_lo/has_hi == 0. */
int tomo_pdtv_iter_slab(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                        const void *p_in_dev[3], void *p_out_dev[3], int dx, int dy, int nz_local,
                        int has_lo, int has_hi, float sigma, float tau, float lt, float theta,
                        int methodTV, int nonneg, int half, void *stream);
/* K iterations (k = 2 or 3) in one pass on a slab whose arrays carry lo_planes / hi_planes in {0, k..3} ghost planes.
 * Ghost planes that must be valid on entry: U and P1..3 k planes below, U k planes and P1..3 k-1 planes above, Input
 * k-1 planes either side.  Result = k applications of tomo_pdtv_iter_slab with ghost refreshes in between, bit for bit.
 * Only the local output planes [z_begin, z_end) are written (0 <= z_begin <= z_end <= nz_local): a rank computes the
 * planes its neighbours wait for first, starts the halo exchange, and computes the interior while the planes travel
 * (tomobar_amd/slab.py).
 * (Which k a run uses is the host's choice: tomobar_amd/slab.py asks tomo_pdtv_iters_per_launch -- 3 for both dual types in the shipped build.) */
int tomo_pdtv_multi_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                               const void *p_in_dev[3], void *p_out_dev[3], int dx, int dy, int nz_local,
                               int lo_planes, int hi_planes, int z_begin, int z_end, int k, float sigma, float tau,
                               float lt, float theta, int methodTV, int nonneg, int half, void *stream);
/* One ROF_TV iteration on a slab whose arrays address [lo_planes + nz_local + hi_planes][dy][dx] with lo_planes in {0, 2}
 * and hi_planes in {0, 1}, for the local output planes [z_begin, z_end) only (boundary planes first, exchange, then the
 * interior). */
int tomo_roftv_iter_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                               int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin, int z_end,
                               float lambda, float tau, int half, void *stream);
/* One NDF iteration (tomo_ndf) on a slab whose arrays address [lo_planes + nz_local + hi_planes][dy][dx] with lo_planes and
 * hi_planes in {0, 1} -- a ghost plane of U exactly where a z-neighbour exists, so the z differences are zero only at the
 * global faces --, for the local output planes [z_begin, z_end) only.  in_dev is read at the output voxels only (its ghost
 * planes need not be valid); u_out_dev must not alias an array the launch reads. */
int tomo_ndf_iter_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                             int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin, int z_end,
                             float lambda, float sigma, float tau, int penalty, void *stream);
/* One Diff4th iteration (tomo_diff4th) on a slab whose arrays address [lo_planes + nz_local + hi_planes][dy][dx] with
 * lo_planes and hi_planes in {0, 2} -- two ghost planes of U exactly where a z-neighbour exists (the stencil has radius 2),
 * so the z index is clamped only at the global faces --, for the local output planes [z_begin, z_end) only.  in_dev is
 * read at the output voxels only (its ghost planes need not be valid); u_out_dev must not alias an array the launch
 * reads. */
int tomo_diff4th_iter_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                                 int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin, int z_end,
                                 float lambda, float sigma, float tau, void *stream);
/* One LLT_ROF iteration (tomo_llt_rof) on a slab laid out as for tomo_diff4th_iter_slab_range: lo_planes and hi_planes in
 * {0, 2} (the stencil has radius 2: E_d at distance 1 needs U at distance 2), the local output planes [z_begin, z_end)
 * only.  The missing backward neighbour of R_3 and the clamped index of E_3 are decided at the faces of these arrays,
 * which are the global faces.  in_dev is read at the output voxels only; u_out_dev must not alias an array the launch
 * reads. */
int tomo_llt_rof_iter_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                                 int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin, int z_end,
                                 float lambda_rof, float lambda_llt, float tau, void *stream);

/* Halo staging for the z-slab exchange ("tomo_halo_exchange"; the reference scales by independent replicas
 * only, Demos/methods_IR_legacy/MultiGPU_demo.py:144-190, so there is no call to replace).  The transport itself stays
 * with the host (torch.distributed / RCCL in tomobar_amd/slab.py, mpi4py or cupy.cuda.nccl for a CuPy caller --
 * INTEGRATION.md section C); what the library provides is the device side: the planes a neighbour needs -- the last or
 * first k planes of U, P1, P2, P3 (each contiguous in its own array) -- gathered into ONE contiguous staging buffer and
 * scattered back, so that an exchange is one send and one receive per neighbour.  Block i occupies
 * [off_i, off_i + bytes[i]) of the staging buffer with off_0 = 0, off_{i+1} = off_i + round_up(bytes[i], 16);
 * tomo_halo_staging_bytes returns the total.  At most 8 blocks per call. */
size_t tomo_halo_staging_bytes(const size_t *bytes, int nblocks);
int tomo_halo_pack(const void *const *src_dev, const size_t *bytes, int nblocks, void *staging_dev, void *stream);
int tomo_halo_unpack(const void *staging_dev, void *const *dst_dev, const size_t *bytes, int nblocks, void *stream);
/* Both directions of an exchange in ONE launch each (no reference counterpart, as above): tomo_halo_pack2 gathers the blocks
 * for rank-1 into msg_down_dev and the blocks for rank+1 into msg_up_dev; tomo_halo_pull2 scatters the message that came from
 * rank-1 (msg_down_dev) and the one from rank+1 (msg_up_dev) into the ghost planes.  Each message has the layout of
 * tomo_halo_staging_bytes over its own block table, at most 8 blocks per direction; a direction with 0 blocks is valid (its
 * pointers may be NULL) and two empty directions launch nothing.  The messages of tomo_halo_pull2 are meant to lie in a
 * neighbour's region mapped by tomo_ipc_region_open: the device-direct transport of tomobar_amd/slab.py, which needs one pack
 * and one pull launch per exchange where tomo_halo_pack / tomo_halo_unpack need two each. */
int tomo_halo_pack2(const void *const *src_down_dev, const size_t *bytes_down, int nblocks_down, void *msg_down_dev,
                    const void *const *src_up_dev, const size_t *bytes_up, int nblocks_up, void *msg_up_dev, void *stream);
int tomo_halo_pull2(const void *msg_down_dev, void *const *dst_down_dev, const size_t *bytes_down, int nblocks_down,
                    const void *msg_up_dev, void *const *dst_up_dev, const size_t *bytes_up, int nblocks_up, void *stream);
/* Device memory that other PROCESSES map (HIP IPC; no reference counterpart: the reference never moves data between its
 * replicas).  tomo_ipc_region_create allocates `bytes` on `device` with a hipMalloc of the library's own -- an IPC handle names
 * a whole allocation, so a piece of a caching allocator's block cannot be exported -- and writes the 64 opaque bytes another
 * process passes to tomo_ipc_region_open, which returns that memory mapped into the caller.  A handle is opened at most once
 * per process and never by the process that created it.  tomo_ipc_region_close unmaps, tomo_ipc_region_destroy frees; the
 * owner destroys a region only after every mapper has stopped reading it (the caller's protocol: tomobar_amd/slab.py).
 * Synchronous host calls; a HIP failure is TOMO_E_RUNTIME / TOMO_E_NOMEM with the HIP error text in tomo_last_error(). */
int tomo_ipc_region_create(int device, size_t bytes, void **base_dev, unsigned char handle[64]);
int tomo_ipc_region_open(int device, const unsigned char handle[64], void **mapped_dev);
int tomo_ipc_region_close(void *mapped_dev);
int tomo_ipc_region_destroy(void *base_dev);
/* How many PD_TV iterations tomo_pdtv fuses into one launch for float32 (half = 0) / binary16 (half != 0) dual fields under
 * the calling thread's kernel variant: a slab driver that wants to be launch-for-launch identical to the whole-volume
 * operator cuts its iterations the same way (tomobar_amd/slab.py: pd_launch_plan) and keeps that many ghost planes. */
int tomo_pdtv_iters_per_launch(int half);
/* How tomo_pdtv cuts `iters` iterations of an nd-dimensional run (dz planes; ignored for nd = 2) into launches under the
 * calling thread's kernel variant: returns the number of launches and writes the iteration count of the first `capacity`
 * of them to k_out (may be NULL).  Pure host code, no kernel is launched; -1 for nd outside {2, 3} or dz < 1. */
int tomo_pdtv_launch_plan(int iters, int nd, int dz, int *k_out, int capacity);

/* ---------------------------------------------------------------- FBP filter
 * tomo_fbp_filter replaces _filtersinc3D_cupy (tomobar/fourier.py:26-78) and generate_filtersinc
 * (cuda_kernels/generate_filtersync.cu:5-82): every row of `rows` x `nu` float32 values is replaced, in place, by
 * irfft( rfft(row) * f ), f = fftshift-ed half-spectrum sinc-ramp of cut-off `cutoff`, unnormalised transforms with
 * `multiplier` (= 1/angles/nu in RecToolsDIRCuPy.FBP) folded into f.  Batched hipFFT; synchronises the stream. */
int tomo_fbp_filter(int device, float *data_dev, size_t rows, int nu, float cutoff, float multiplier, void *stream);

/* ---------------------------------------------------------------- Fourier reconstruction
 * tomo_fourier_inv replaces the device side of RecToolsDIRCuPy.FOURIER_INV (tomobar/methodsDIR_CuPy.py:152-447: the
 * stages _fbp_filtering :449-545, _setup_backprojection_input :645-683, _fft_and_interpolation :701-836,
 * ifft_gathered_projections :851-897, unpad_reconstructed_data :920-967) and the kernels of
 * tomobar/cuda_kernels/fft_us_kernels.cu.
 *   data_dev  [nz][nproj][raw_n] float32, nz and raw_n even (the caller pads odd sizes as the reference does, :265-279)
 *   out_dev   [out_z][out_size][out_size] float32; out_z = nz or nz-1 (odd original height)
 *   n         detector width after horizontal padding (even), ne the oversampled filter width (:465-474)
 *   unpad_m   first reconstructed column/row relative to -n/2 (unpad_recon_m, :933)
 *   w_host    HOST array of ne/2+1 complex64 (re,im pairs): filter table x phase ramp of the rotation axis (:481-483)
 *   theta_host HOST array of nproj float32 angles as the kernels see them (= -AnglesVec, :295)
 *   m, mu     footprint half-width and Gaussian parameter (:321-322, :726-737)
 *   center_size  min(center_size, 2n) of the reference (:290): >= 192 selects the circular-support gathering inside
 *             the centre box and the square-footprint form outside it; < 192 the square-footprint form everywhere.
 * Workspace: the per-device scratch arena; hipFFT plans are cached between calls (both released by
 * tomo_release_scratch).  Processes 128 slices per chunk, synchronises the stream before returning. */
int tomo_fourier_inv(int device, const float *data_dev, float *out_dev, int nz, int out_z, int nproj, int raw_n,
                     int n, int ne, int unpad_m, int out_size, const float *w_host, const float *theta_host,
                     int m, float mu, int center_size, void *stream);
/* libtomo_mi355x_dev.so alone also exports tomo_fourier_gather, the gathering launch of the pipeline above on the caller's
 * arrays (deliberately not declared: the shipped library has no such symbol; tomobar_amd/_lib.py DEV_SIGNATURES binds it where
 * it exists).  Arguments, in order: int device; const float *g_dev, the polar samples as float2 [nproj][n][64] with the
 * slice pair fastest; float *f_dev, the frequency grid as float2 [zc][2n][2n], every element of which is written (checkerboard
 * sign of the first 2D shift included); int zc in 1..64; int nproj, n, m; float mu; int center_size; const float
 * *theta_host; void *stream.  Same checks, same host tables (cosf / sinf, stable sort, in the scratch arena) and same launch
 * as tomo_fourier_inv: one function each in csrc/fourier_inv.hip, called by both.  Synchronises the stream. */

/* kernel-variant selector (per calling host thread): name in {"bp","fp","pdtv","roftv"}; variant 0 = the default of every
 * class.  The shipped library accepts two other values: "fp" 5 = the default kernels, but tomo_ctx_volume_zquad_ok answers no,
 * so a driver keeps the planar X_t (the A/B switch of TOMO_VOLUME_ZQUAD: one process runs both ways), and "pdtv" 22 = float32 duals with the rounding sequence of the
 * reference's kernels reproduced bit for bit (primal_dual_for_total_variation.cu:66-123; FMA-corrected 1 / sqrtf and
 * quotient), +5 ... +16 % per launch depending on the box.  The default runs float32 duals with relaxed arithmetic (v_rsq_f32 instead of 1 / sqrtf, a
 * host-computed 1 / (1 + lt) instead of the divide: within 1e-5 of the reference, typically 3e-7); binary16 duals
 * (half_precision) and ROF_TV reproduce the reference's roundings in every build (rudin_osher_fatemi_total_variation.cu:51-61).
 * Anything else returns TOMO_E_INVALID: the independent implementations and A/B builds used by tests/ and tools/ (bp 1/2,
 * fp 1/2/3, pdtv 1/2/3/21, roftv 1..4) and the measurement switches ("probe") exist only in libtomo_mi355x_dev.so
 * (csrc/Makefile: `make dev`). */
int tomo_set_variant(const char *kernel, int variant);

/* In-library kernel timing for bench.py's roofline object: while enabled, every launch group of a kernel class
 * ("bp","fp","pdtv","roftv") is bracketed by HIP events recorded ON THE LAUNCH STREAM.  tomo_profile_read
 * synchronises those events and returns the number of kernel launches and their summed duration. */
int tomo_profile_enable(int on);
int tomo_profile_read(const char *kernel, long long *launches, double *total_ms);

/* ---------------------------------------------------------------- host (CPU) 2D plumbing, BASELINE configs[0]
 * RecToolsDIR(..., device_projector="cpu") of the reference runs ASTRA's CPU `line` projector / `BP` algorithm
 * (tomobar/methodsDIR.py:71-175, astra_base.py:224-232,310-372).  These two entry points take HOST pointers and need no
 * GPU: img [n][n], sino [na][nu], angles in radians, scalar CoR (the reference's CPU path rejects a non-zero one,
 * astra_base.py:150-153).  Same operator model and float32 arithmetic as tomo_bp3d / tomo_fp3d. */
int tomo_host_bp2d(const float *sino_host, float *img_host, int n, int nu, int na, const double *angles_host, double cor);
int tomo_host_fp2d(const float *img_host, float *sino_host, int n, int nu, int na, const double *angles_host, double cor);

#ifdef __cplusplus
}
#endif
#endif /* TOMO_MI355X_H */
