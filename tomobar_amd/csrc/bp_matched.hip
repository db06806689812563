// Matched back projector for gfx950: the exact transpose of the Joseph forward projector of proj_kernels.hip
// (fp_tiled.inl), with the FISTA / ADMM epilogues of the shipped (unmatched) back projector fused in.
//
// Why a gather at the shipped taps is A^T (docs/kernels/bp_matched.md): in the forward projector the voxel `iy` of column
// `ix` receives the tent weight max(0, 1 - |f_y - iy|) / |sin| from detector pixel `iu` (x-stepping angle).  f_y is affine
// in iu with slope 1/sin and equals iy exactly at iu* = f, the detector coordinate of the voxel that the shipped back
// projector computes.  The tent therefore has half-width |sin| <= 1 detector pixels: it can cover only i0 = floor(f) and
// i0 + 1.  With w = f - i0 and q = 1 / max(|sin|, |cos|) (tomo_angle_t::scale) the two weights are
//     w0 = max(1 - w q, 0) q            w1 = max(1 - (1 - w) q, 0) q
// where the shipped projector uses 1 - w and w.  The y-stepping case is the same with cos.  One float32 rounding per
// operation, in this order; angles ascending, tap 0 then tap 1, fmaf: tests/_matched_bp_oracle.py restates it bit for bit.
//
// Kernel: the brick of bp_brick.inl in its planar-input form -- the taps are the same, hence so are the windows.  A
// 256-thread workgroup owns a 32(x) x 16(y) x 16(z) voxel brick, a wave a 16 x 4 patch, a thread two voxel columns (rows
// four apart) x 16 slices.  Per batch of 8 angles the <= 37 detector samples the brick can touch are staged through
// registers into LDS as float4 over z (the loads of batch b + 1 are in flight while batch b is sampled), every tap is one
// ds_read_b128 serving four slices.  New per (voxel column, angle): q from the angle record and six VALU operations that
// turn w into (w0, w1), shared by the 16 slices of the column.
// The argument struct, the epilogue arithmetic (bp_value) and the host front end are those of the shipped back projector:
// bp_common.h.
#include "bp_common.h"

#include <string>

namespace {

constexpr int MB_TX = 32, MB_TY = 16, MB_ZQ = 4, MB_AB = 8;
// columns per (angle, z-quad) row of the tile: a brick sees at most 31|cos| + 15|sin| <= 34.5 detector pixels plus the
// second tap and the floor = 37; 40 makes the staging 5 items per thread exactly
constexpr int MB_PITCH = 40;
constexpr int MB_NITEMS = MB_AB * MB_ZQ * MB_PITCH;
constexpr int MB_ITEMS = MB_NITEMS / 256;
static_assert(MB_NITEMS == 256 * MB_ITEMS, "staging items must divide evenly");

// The epilogues: the loads and stores around bp_value.
template <int EPI>
__device__ __forceinline__ void mb_epilogue(const BpArgs &a, size_t idx, float g)
{
    float o0 = 0.0f, o1 = 0.0f;
    if (EPI == EPI_PLAIN) {
        a.vol[idx] = g;
    } else if (EPI == EPI_FISTA) {
        bp_value<EPI>(a, g, a.xt[idx], 0.0f, 0.0f, o0, o1);
        a.xout[idx] = o0;
    } else if (EPI == EPI_FISTA_MOM) {
        bp_value<EPI>(a, g, a.xt[idx], a.xold[idx], 0.0f, o0, o1);
        a.xout[idx] = o0;
        a.xt_out[idx] = o1;
    } else {
        bp_value<EPI>(a, g, a.xout[idx], a.xold[idx], a.xt[idx], o0, o1);
        a.xout[idx] = o0;
        a.xt_out[idx] = o1;
    }
}

// the same on four consecutive voxels of a row (idx a multiple of 4, 16-byte aligned arrays): one dwordx4 access per
// array.  Non-temporal, like the shipped epilogue: the volume streams are touched once and must not evict the sinogram
// windows that every brick of the XCD re-reads from L2.  Fused forms only: plain stores gain nothing from the hand-over.
template <int EPI>
__device__ __forceinline__ void mb_epilogue4(const BpArgs &a, size_t idx, v4f g)
{
    static_assert(EPI != EPI_PLAIN, "the plain epilogue stores its accumulators directly");
    auto ld4 = [&](const float *p) { return __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p + idx)); };
    auto st4 = [&](float *p, v4f v) { __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(p + idx)); };
    const v4f zero = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    v4f i0 = zero, i1 = zero, i2 = zero, o0 = zero, o1 = zero;
    if (EPI == EPI_FISTA) {
        i0 = ld4(a.xt);
    } else if (EPI == EPI_FISTA_MOM) {
        i0 = ld4(a.xt); i1 = ld4(a.xold);
    } else if (EPI == EPI_ADMM) {
        i0 = ld4(a.xout); i1 = ld4(a.xold); i2 = ld4(a.xt);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float p = 0.0f, r = 0.0f;
        bp_value<EPI>(a, g[k], i0[k], i1[k], i2[k], p, r);
        o0[k] = p; o1[k] = r;
    }
    st4(a.xout, o0);
    if (EPI != EPI_FISTA) st4(a.xt_out, o1);
}

template <int EPI>
__global__ __launch_bounds__(256) void bp_matched_kernel(BpArgs a)
{
    // the double-buffered tile [2][angle][z-quad][u] (2 x 20 KiB), then the window table (three slots: a slow wave may
    // still sample batch b - 1 while the window of batch b + 1 is written)
    __shared__ float4 mb_smem[2 * MB_NITEMS + (3 * MB_AB * 4 + 15) / 16];
    float4(*tile2)[MB_NITEMS] = reinterpret_cast<float4(*)[MB_NITEMS]>(mb_smem);
    int(*umin_s)[MB_AB] = reinterpret_cast<int(*)[MB_AB]>(mb_smem + 2 * MB_NITEMS);

    // workgroup b lands on XCD b % 8: every XCD gets one contiguous eighth of the (z-brick, tile) list, so the sinogram
    // rows of a z-brick stay in that XCD's L2
    const int ntiles = a.ntx * a.nty;
    const int b = blockIdx.x, xcd = b & 7, qb = b >> 3;
    const int per_xcd = (a.nzb * ntiles + 7) >> 3;
    const int wi = xcd * per_xcd + qb;
    if (wi >= a.nzb * ntiles) return;  // uniform for the workgroup
    const int zb = wi / ntiles;
    const int tq = wi % ntiles;
    const int tx0 = (tq % a.ntx) * MB_TX, ty0 = (tq / a.ntx) * MB_TY;
    const int z0 = zb * (4 * MB_ZQ);

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ix = tx0 + (wave & 1) * 16 + (lane & 15);
    const int iy0 = ty0 + (wave >> 1) * 8 + (lane >> 4);  // rows iy0 and iy0 + 4
    const float half_n = 0.5f * (float)a.n - 0.5f, half_u = 0.5f * (float)a.nu - 0.5f;
    const float xw = (float)ix - half_n;
    const float yw0 = (float)iy0 - half_n, yw1 = (float)(iy0 + 4) - half_n;

    // accumulators as explicit 2-vectors (slices 2h, 2h + 1): one v_pk_fma_f32 per tap and slice pair
    v2f acc[2][2 * MB_ZQ];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 2 * MB_ZQ; ++j) acc[r][j] = v2f{0.0f, 0.0f};

    // ---- loop-invariant part of the staging items: item = tid + 256 m  ->  (angle slot, z-quad, column)
    const unsigned zstride = (unsigned)a.na * (unsigned)a.nu;  // elements; the host guarantees 16 * zstride * 4 < 2^32
    const int zlim = a.nz - 1 - z0;                            // last valid slice relative to z0 (>= 0)
    const bool ragged = zlim < 4 * MB_ZQ - 1;                  // uniform: only the last z-brick
    int it_aa[MB_ITEMS], it_j[MB_ITEMS];
    unsigned it_off[MB_ITEMS];  // element offset of (slice z0 + 4 zq, angle slot, column 0) from the batch base
#pragma unroll
    for (int m = 0; m < MB_ITEMS; ++m) {
        const int item = tid + 256 * m;
        it_j[m] = item % MB_PITCH;
        const int zq = (item / MB_PITCH) % MB_ZQ;
        it_aa[m] = item / (MB_PITCH * MB_ZQ);
        it_off[m] = (unsigned)min(4 * zq, zlim) * zstride + (unsigned)it_aa[m] * (unsigned)a.nu;
    }
    const float *sino_z0 = a.sino + (size_t)z0 * zstride;

    auto window = [&](int a0, int buf) {  // detector window of the brick for the 8 angles of a batch
        if (tid < MB_AB) {
            // the coordinate is monotone in x and in y, so the four corners bound it
            const tomo_angle_t t = a.tab[min(a0 + tid, a.na - 1)];
            const float off = half_u - t.cor;
            const float x0 = (float)tx0 - half_n, x1 = (float)(tx0 + MB_TX - 1) - half_n;
            const float y0 = (float)ty0 - half_n, y1 = (float)(ty0 + MB_TY - 1) - half_n;
            const float f00 = fmaf(x0, t.cs, fmaf(y0, t.sn, off)), f10 = fmaf(x1, t.cs, fmaf(y0, t.sn, off));
            const float f01 = fmaf(x0, t.cs, fmaf(y1, t.sn, off)), f11 = fmaf(x1, t.cs, fmaf(y1, t.sn, off));
            // clamp so that the int conversion and the offsets below stay in range whatever the geometry
            const float lo = fminf(fminf(f00, f10), fminf(f01, f11));
            umin_s[buf][tid] = (int)fminf(fmaxf(floorf(lo), -1.0e6f), 1.0e6f);
        }
    };

    float4 pre[MB_ITEMS];
    auto prefetch = [&](int a0, int buf) {  // batch a0 -> registers (zero outside the detector)
        const float *base = sino_z0 + (size_t)a0 * a.nu;
        const int amax = a.na - 1 - a0;  // angle slots beyond the subset re-read the last angle (never sampled)
#pragma unroll
        for (int m = 0; m < MB_ITEMS; ++m) {
            const int u = umin_s[buf][it_aa[m]] + it_j[m];
            const unsigned mk = (u >= 0 && u < a.nu) ? 0xffffffffu : 0u;
            unsigned off = it_off[m] + (unsigned)min(max(u, 0), a.nu - 1);
            if (it_aa[m] > amax) off -= (unsigned)(it_aa[m] - amax) * (unsigned)a.nu;
            float4 v;
            if (!ragged) {
                v.x = base[off];
                v.y = base[off + zstride];
                v.z = base[off + 2 * zstride];
                v.w = base[off + 3 * zstride];
            } else {  // slices past the end of the volume are fed by the last valid one; their accumulators are not stored
                const int zrel = min(4 * (((tid + 256 * m) / MB_PITCH) % MB_ZQ), zlim);
                v.x = base[off];
                v.y = base[off + (unsigned)(min(zrel + 1, zlim) - zrel) * zstride];
                v.z = base[off + (unsigned)(min(zrel + 2, zlim) - zrel) * zstride];
                v.w = base[off + (unsigned)(min(zrel + 3, zlim) - zrel) * zstride];
            }
            v.x = __uint_as_float(__float_as_uint(v.x) & mk);
            v.y = __uint_as_float(__float_as_uint(v.y) & mk);
            v.z = __uint_as_float(__float_as_uint(v.z) & mk);
            v.w = __uint_as_float(__float_as_uint(v.w) & mk);
            pre[m] = v;
        }
    };

    if (a.na > 0) window(0, 0);  // (an empty subset reads nothing: its gradient is zero)
    __syncthreads();
    if (a.na > 0) prefetch(0, 0);
    int buf = 0;
    for (int a0 = 0; a0 < a.na; a0 += MB_AB, buf = (buf == 2 ? 0 : buf + 1)) {
        const int nb = min(MB_AB, a.na - a0);
        const bool more = a0 + MB_AB < a.na;
        const int nbuf = (buf == 2 ? 0 : buf + 1);
        if (more) window(a0 + MB_AB, nbuf);
        // double-buffered tile: waves still sampling batch b - 1 read the other buffer, so one barrier per batch is enough
        float4 *tile = tile2[(a0 / MB_AB) & 1];
#pragma unroll
        for (int m = 0; m < MB_ITEMS; ++m) tile[tid + 256 * m] = pre[m];
        __syncthreads();  // tile b and the window of batch b + 1 visible; everyone is past the sampling of batch b - 1
        if (more) prefetch(a0 + MB_AB, nbuf);  // in flight while this batch is sampled
        auto sample = [&](int aa) {
            const tomo_angle_t t = a.tab[a0 + aa];  // wave-uniform: scalar loads
            const float off = half_u - t.cor, q = t.scale;
            const int um = umin_s[buf][aa];
            // the window origin is wave-uniform: fold it into a scalar byte offset so that a tap address is one v_lshl_add
            int ab = __builtin_amdgcn_readfirstlane((aa * (MB_ZQ * MB_PITCH) - um) * 16);
            asm("" : "+s"(ab));  // opaque: otherwise the * 16 is factored back out (a second VALU op per tap)
            const char *tb = reinterpret_cast<const char *>(tile);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float f = fmaf(xw, t.cs, fmaf(r ? yw1 : yw0, t.sn, off));
                const float fl = floorf(f);
                const float w = lerp_w<false>(f, fl);
                // the transposed Joseph weights (one rounding per operation, in this order)
                const float w0 = fmaxf(1.0f - w * q, 0.0f) * q;
                const float w1 = fmaxf(1.0f - (1.0f - w) * q, 0.0f) * q;
                const int idx = (int)fl;
                const v2f w0v = v2f{w0, w0}, w1v = v2f{w1, w1};
#pragma unroll
                for (int zq = 0; zq < MB_ZQ; ++zq) {
                    const v4f *tap = reinterpret_cast<const v4f *>(tb + ((idx << 4) + ab)) + zq * MB_PITCH;
                    const v4f s0 = tap[0], s1 = tap[1];
                    v2f &c0 = acc[r][zq * 2], &c1 = acc[r][zq * 2 + 1];
                    c0 = __builtin_elementwise_fma(w0v, s0.lo, c0); c0 = __builtin_elementwise_fma(w1v, s1.lo, c0);
                    c1 = __builtin_elementwise_fma(w0v, s0.hi, c1); c1 = __builtin_elementwise_fma(w1v, s1.hi, c1);
                }
            }
        };
        if (nb == MB_AB) {  // unrolled: the 8 angle records become one block of scalar loads ahead of the sampling
#pragma unroll
            for (int aa = 0; aa < MB_AB; ++aa) sample(aa);
        } else {
            for (int aa = 0; aa < nb; ++aa) sample(aa);
        }
    }
    // ---- epilogue.  A brick that lies inside the volume hands its accumulators over through LDS (the tile buffers are
    // free now) so that a lane owns four consecutive voxels of a row: dwordx4 accesses in whole 128-byte lines.
    if constexpr (EPI != EPI_PLAIN) {  // (plain stores gain nothing from the hand-over)
        if ((tx0 + MB_TX <= a.n) && (ty0 + MB_TY <= a.n) && (z0 + 4 * MB_ZQ <= a.nz) && ((a.n & 3) == 0) && a.epi_aligned) {  // uniform for the workgroup
            float *stg = reinterpret_cast<float *>(&tile2[0][0]);  // [16 z][16 y][32 x] floats = 32 KiB of the 40
            __syncthreads();  // every wave is past the sampling of the last batch
            const int xr = ix - tx0, yr = iy0 - ty0;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 4 * MB_ZQ; ++j) stg[(j * MB_TY + yr + 4 * r) * MB_TX + xr] = acc[r][j >> 1][j & 1];
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 4 * MB_ZQ * MB_TY * (MB_TX / 4) / 256; ++m) {
                const int item = tid + 256 * m;  // float4 index = (z * 16 + y) * 8 + x4
                const int x4 = item & (MB_TX / 4 - 1), yy = (item / (MB_TX / 4)) & (MB_TY - 1), zz = item / (MB_TX / 4 * MB_TY);
                const v4f g = reinterpret_cast<const v4f *>(stg)[item];
                mb_epilogue4<EPI>(a, ((size_t)(z0 + zz) * a.n + (ty0 + yy)) * a.n + tx0 + 4 * x4, g);
            }
            return;
        }
    }
    if (ix < a.n) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int iy = iy0 + 4 * r;
            if (iy < a.n) {
#pragma unroll
                for (int j = 0; j < 4 * MB_ZQ; ++j)
                    if (z0 + j < a.nz) mb_epilogue<EPI>(a, ((size_t)(z0 + j) * a.n + iy) * a.n + ix, acc[r][j >> 1][j & 1]);
            }
        }
    }
}

// what the matched kernel refuses beyond bp_prepare
int mb_check(const tomo_ctx *ctx, const BpArgs &a)
{
    TOMO_REQUIRE((ctx->flags & TOMO_FLAG_LERP8) == 0,
                 "the matched back projector is the transpose of the unquantised forward projector: no transpose is defined "
                 "for a context created with TOMO_FLAG_LERP8");
    TOMO_REQUIRE(ctx->res_layout == TOMO_RESIDUAL_PLANAR,
                 "the matched back projector reads the planar [nz][subset_size][nu] layout only: set TOMO_RESIDUAL_PLANAR first");
    // the kernel addresses a 16-slice sinogram slab with 32-bit element offsets
    TOMO_REQUIRE((long)a.na * a.nu < (1L << 27), "matched back projection: angles x detector >= 2^27 samples per slice");
    return TOMO_OK;
}

template <int EPI>
int mb_launch(tomo_ctx *ctx, BpArgs a, hipStream_t st)
{
    TOMO_ON_DEVICE(ctx->device);
    tomo_prof_scope prof(PROF_BP, st, 1);
    a.epi_aligned = bp_epi_aligned<EPI>(a);
    a.ntx = ceil_div(a.n, MB_TX);
    a.nty = ceil_div(a.n, MB_TY);
    a.nzb = ceil_div(a.nz, 4 * MB_ZQ);
    const long blocks = 8L * (((long)a.nzb * a.ntx * a.nty + 7) / 8);
    if (blocks > 0x7fffffffL) return tomo_fail(TOMO_E_INVALID, "volume too large for one BP launch");
    ctx->last_bp_path = "matched brick(32x16x16, planar staging)";
    if (blocks > 0) bp_matched_kernel<EPI><<<(unsigned)blocks, 256, 0, st>>>(a);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

}  // namespace

// ---- entry points: bp_prepare, the form's filler (bp_common.h), mb_check, mb_launch
extern "C" int tomo_bp3d_matched(tomo_ctx *ctx, int subset, const float *sino_dev, float *vol_dev, void *stream)
{
    BpArgs a;
    int rc = bp_prepare(ctx, subset, sino_dev, a);
    if (rc == TOMO_OK) rc = bp_fill_plain(a, vol_dev);
    if (rc == TOMO_OK) rc = mb_check(ctx, a);
    if (rc != TOMO_OK) return rc;
    return mb_launch<EPI_PLAIN>(ctx, a, as_stream(stream));
}

extern "C" int tomo_bp3d_matched_fista(tomo_ctx *ctx, int subset, const float *res_dev, const float *xt_dev,
                                       float *xout_dev, float l_inv, int nonneg, void *stream)
{
    BpArgs a;
    int rc = bp_prepare(ctx, subset, res_dev, a);
    if (rc == TOMO_OK) rc = bp_fill_fista(a, xt_dev, xout_dev, l_inv, nonneg);
    if (rc == TOMO_OK) rc = mb_check(ctx, a);
    if (rc != TOMO_OK) return rc;
    return mb_launch<EPI_FISTA>(ctx, a, as_stream(stream));
}

extern "C" int tomo_bp3d_matched_fista_momentum(tomo_ctx *ctx, int subset, const float *res_dev, float *xt_dev,
                                                float *xold_x_dev, float l_inv, float beta, int nonneg, void *stream)
{
    BpArgs a;
    int rc = bp_prepare(ctx, subset, res_dev, a);
    if (rc == TOMO_OK) rc = bp_fill_fista_momentum(a, xt_dev, xold_x_dev, l_inv, beta, nonneg);
    if (rc == TOMO_OK) rc = mb_check(ctx, a);
    if (rc != TOMO_OK) return rc;
    return mb_launch<EPI_FISTA_MOM>(ctx, a, as_stream(stream));
}

extern "C" int tomo_bp3d_matched_admm(tomo_ctx *ctx, int subset, const float *res_dev, float *z_dev, const float *x_dev,
                                      const float *u_dev, float *zu_out_dev, float tau, float rho, int relax_on,
                                      float one_minus_alpha, float alpha, int nonneg, void *stream)
{
    BpArgs a;
    int rc = bp_prepare(ctx, subset, res_dev, a);
    if (rc == TOMO_OK) rc = bp_fill_admm(a, z_dev, x_dev, u_dev, zu_out_dev, tau, rho, relax_on, one_minus_alpha, alpha, nonneg);
    if (rc == TOMO_OK) rc = mb_check(ctx, a);
    if (rc != TOMO_OK) return rc;
    return mb_launch<EPI_ADMM>(ctx, a, as_stream(stream));
}
