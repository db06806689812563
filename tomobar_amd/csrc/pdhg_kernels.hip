// The three launches PDHG (primal-dual hybrid gradient, Chambolle-Pock, on the reconstruction problem itself:
//     min_x F(Ax) + lambda TV(x)  [+ x >= 0],   F = 1/2 |. - b|^2, |. - b|_1 or the Kullback-Leibler term)
// adds to the forward projector and the matched back projector for gfx950.  There is no reference implementation in the
// tree: what is computed is the algorithm stated in docs/kernels/pdhg.md, formula-level parity, unpinned --
// tests/_pdhg_oracle.py restates it in numpy and the kernels reproduce its float32 form bit for bit (one rounding per
// operation in the stated order, no FMA contraction: -ffp-contract=off and no fmaf here; sqrtf and / are the compiler's
// correctly rounded ones).
//
//   pdhg_sino_kernel    step 2: the prox of the conjugate of the data term on the sinogram dual y, element-wise, in place
//   pdhg_dual_kernel    step 4: q_d += sigma F_d(x-bar), projected onto the ball (isotropic) or the box (anisotropic)
//   pdhg_primal_kernel  step 5: x' = x - tau (g - div q) [clamped], x-bar = 2 x' - x
// The last two are plane marches on the skeleton of tgv_dual.inl / tgv_primal.inl (4 rows per lane, 2 x 2 waves, 63
// columns per wave; the wave shifts, the plane I/O, the z-march grid and the array skew are the one copy in
// zmarch_common.h).  Each voxel's own q, x are read by that voxel only, and the neighbours a launch reads belong to fields
// it does not write, so nothing is ping-ponged.  Algorithmic traffic in 3D: dual 4 + 3 x 8 = 28 B, primal 3 x 4 + 8 + 8 =
// 28 B per voxel and iteration; the sinogram kernel moves 16 B per sample.
#include "zmarch_common.h"

namespace {

struct PdhgArgs {
    float *x, *xb;     // the primal variable and its extrapolation x-bar
    const float *g;    // A^T y
    float *q[3];       // the TV dual (q[0] null: no TV block)
    int dx, dy, dz;
    float sigma, tau, lambda;
    int nonneg;
};

// ------------------------------------------------------------------------------------------ step 2: the sinogram dual
template <int MODE>
__device__ __forceinline__ float pdhg_sino_one(float y, float r, float b, float sigma, float one_sigma, float c4)
{
    if (MODE == TOMO_PDHG_LS) return (y + sigma * (r - b)) / one_sigma;
    if (MODE == TOMO_PDHG_L1) {
        const float v = y + sigma * (r - b);
        return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    }
    const float v = y + sigma * r;
    const float t = v - 1.0f;
    const float bp = b > 0.0f ? b : 0.0f;
    return 0.5f * ((1.0f + v) - sqrtf(t * t + c4 * bp));
}

constexpr int SINO_BLOCK = 256;
constexpr int SINO_MAX_GRID = 256 * 8;   // 256 CUs x 8 blocks, grid-stride beyond

// VEC: 16-byte accesses over the first n / 4 quads and a scalar tail by block 0 (all three arrays 16-byte aligned)
template <int MODE, bool VEC>
__global__ __launch_bounds__(SINO_BLOCK) void pdhg_sino_kernel(float *y, const float *r, const float *b, size_t n,
                                                               float sigma, float one_sigma, float c4)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const size_t n4 = n >> 2;
        for (size_t i = first; i < n4; i += stride) {
            float4 vy = reinterpret_cast<const float4 *>(y)[i];
            const float4 vr = reinterpret_cast<const float4 *>(r)[i];
            const float4 vb = reinterpret_cast<const float4 *>(b)[i];
            vy.x = pdhg_sino_one<MODE>(vy.x, vr.x, vb.x, sigma, one_sigma, c4);
            vy.y = pdhg_sino_one<MODE>(vy.y, vr.y, vb.y, sigma, one_sigma, c4);
            vy.z = pdhg_sino_one<MODE>(vy.z, vr.z, vb.z, sigma, one_sigma, c4);
            vy.w = pdhg_sino_one<MODE>(vy.w, vr.w, vb.w, sigma, one_sigma, c4);
            reinterpret_cast<float4 *>(y)[i] = vy;
        }
        const size_t i = (n4 << 2) + threadIdx.x;
        if (blockIdx.x == 0 && i < n) y[i] = pdhg_sino_one<MODE>(y[i], r[i], b[i], sigma, one_sigma, c4);
    } else {
        for (size_t i = first; i < n; i += stride) y[i] = pdhg_sino_one<MODE>(y[i], r[i], b[i], sigma, one_sigma, c4);
    }
}

template <int MODE>
static void pdhg_sino_launch(float *y, const float *r, const float *b, size_t n, float sigma, hipStream_t st)
{
    const bool vec = ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
    const size_t items = vec ? (n >> 2) : n;
    size_t grid = (items + SINO_BLOCK - 1) / SINO_BLOCK;
    if (grid < 1) grid = 1;
    if (grid > (size_t)SINO_MAX_GRID) grid = SINO_MAX_GRID;
    const float one_sigma = 1.0f + sigma, c4 = 4.0f * sigma;
    if (vec)
        pdhg_sino_kernel<MODE, true><<<(unsigned)grid, SINO_BLOCK, 0, st>>>(y, r, b, n, sigma, one_sigma, c4);
    else
        pdhg_sino_kernel<MODE, false><<<(unsigned)grid, SINO_BLOCK, 0, st>>>(y, r, b, n, sigma, one_sigma, c4);
}

// ------------------------------------------------------------------------------------------ step 4: the TV dual
// A lane owns RY rows of one x column and walks z.  The +x neighbour is the next lane (lane 63 of a wave is a halo lane:
// 63 columns per wave), the +y neighbour the next register (one halo row below the tile), the +z neighbour the plane loaded
// one step ahead, which becomes the current plane of the next step: x-bar is read once per launch (plus halos), q read and
// written once.
template <int ND, bool ANISO, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void pdhg_dual_kernel(PdhgArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
{
    // XCD banding of rof_zmarch.inl: every XCD owns one contiguous eighth of the row-major tile list
    const int j = (int)blockIdx.x >> 3;
    const int xcd = (int)blockIdx.x & 7;
    const int tq = xcd * tiles_per_xcd + (j % tiles_per_xcd);
    const int chunk = j / tiles_per_xcd;
    if (tq >= gx * gy) return;
    const int xb = tq % gx;
    const int yb = tq / gx;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int x = (xb * WX + (wave % WX)) * 63 + lane;
    const int y0 = (yb * WY + (wave / WX)) * RY;
    const int dx = a.dx, dy = a.dy, dz = a.dz;
    const int zc0 = chunk * zchunk;
    const int zc1 = min(zc0 + zchunk, dz);
    if (zc0 >= zc1) return;

    const size_t sz = (size_t)dx * dy;
    const bool emit_lane = (lane < 63) && (x < dx);
    const bool x_next = x < dx - 1;
    const unsigned xo = (unsigned)min(x, dx - 1) * 4u;   // the clamped column: every load stays inside the plane
    const int wy0 = __builtin_amdgcn_readfirstlane(y0);
    const int pitch = dx * 4;
    const PlaneIO io{(int)(sz * 4)};
    // slot q = row y0 + q (q = RY: the halo row), clamped into the plane
    auto rowoff = [&](int q) __attribute__((always_inline)) { return min(wy0 + q, dy - 1) * pitch; };

    float cur[RY + 1], nxt[RY + 1];
#pragma unroll
    for (int q = 0; q <= RY; ++q) cur[q] = io.ld(a.xb + sz * zc0, xo, rowoff(q));

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_next = t < dz - 1;
        if (ND == 3) {
            const size_t pn = sz * min(t + 1, dz - 1);
#pragma unroll
            for (int q = 0; q <= RY; ++q) nxt[q] = io.ld(a.xb + pn, xo, rowoff(q));
        }
        float Q[ND][RY];
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int r = 0; r < RY; ++r) Q[d][r] = io.ld(a.q[d] + sz * t, xo, rowoff(r));

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_next = y0 + r < dy - 1;
            // F_d(x-bar): a[i + e_d] - a[i], exactly 0 on the last index of the axis
            const float c = cur[r];
            const float cx = wave_next(c);
            float F[3];
            F[0] = x_next ? cx - c : 0.0f;
            F[1] = y_next ? cur[r + 1] - c : 0.0f;
            F[2] = (ND == 3 && z_next) ? nxt[r] - c : 0.0f;
#pragma unroll
            for (int d = 0; d < ND; ++d) Q[d][r] = Q[d][r] + a.sigma * F[d];
            if (ANISO) {
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    const float v = Q[d][r] < -a.lambda ? -a.lambda : Q[d][r];
                    Q[d][r] = v > a.lambda ? a.lambda : v;
                }
            } else {
                float m = Q[0][r] * Q[0][r] + Q[1][r] * Q[1][r];
                if (ND == 3) m = m + Q[ND - 1][r] * Q[ND - 1][r];
                const float n = sqrtf(m) / a.lambda;
                const float den = n > 1.0f ? n : 1.0f;   // q / 1 is q: the same bits as leaving it alone
#pragma unroll
                for (int d = 0; d < ND; ++d) Q[d][r] = Q[d][r] / den;
            }
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) {
#pragma unroll
                for (int d = 0; d < ND; ++d) io.st(a.q[d] + sz * t, xo, rowoff(r), Q[d][r]);
            }
        }
        if (ND == 3) {
#pragma unroll
            for (int q = 0; q <= RY; ++q) cur[q] = nxt[q];
        }
    }
}

// ------------------------------------------------------------------------------------------ step 5: the primal
// The mirror image: the -x neighbour is the previous lane (lane 0 of a wave is the halo lane), the -y neighbour the previous
// register (one halo row above the tile, q2 only), the -z neighbour the carried registers of the plane before (q3; a
// z-chunk loads them once for the plane below its first).  q and g are read and not written; x is read and x, x-bar are
// written at the lane's own voxels only.  TV = false drops the q loads: div is 0.
template <int ND, bool TV, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void pdhg_primal_kernel(PdhgArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
{
    const int j = (int)blockIdx.x >> 3;
    const int xcd = (int)blockIdx.x & 7;
    const int tq = xcd * tiles_per_xcd + (j % tiles_per_xcd);
    const int chunk = j / tiles_per_xcd;
    if (tq >= gx * gy) return;
    const int xb = tq % gx;
    const int yb = tq / gx;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int x = (xb * WX + (wave % WX)) * 63 - 1 + lane;
    const int y0 = (yb * WY + (wave / WX)) * RY;
    const int dx = a.dx, dy = a.dy, dz = a.dz;
    const int zc0 = chunk * zchunk;
    const int zc1 = min(zc0 + zchunk, dz);
    if (zc0 >= zc1) return;

    const size_t sz = (size_t)dx * dy;
    const bool emit_lane = (lane > 0) && (x < dx);
    const bool x_prev = x > 0;
    const unsigned xo = (unsigned)min(max(x, 0), dx - 1) * 4u;   // the clamped column: every load stays inside the plane
    const int wy0 = __builtin_amdgcn_readfirstlane(y0);
    const int pitch = dx * 4;
    const PlaneIO io{(int)(sz * 4)};
    // slot q = row y0 - 1 + q (q = 0: the halo row), clamped into the plane
    auto rowoff = [&](int q) __attribute__((always_inline)) { return min(max(wy0 - 1 + q, 0), dy - 1) * pitch; };

    // the plane below: q3
    float Zp[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) Zp[r] = 0.0f;
    if (TV && ND == 3 && zc0 > 0) {
#pragma unroll
        for (int r = 0; r < RY; ++r) Zp[r] = io.ld(a.q[ND - 1] + sz * (zc0 - 1), xo, rowoff(r + 1));
    }

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_prev = t > 0;
        const size_t pt = sz * t;
        float Q1[RY], Q2[RY + 1], Q3[RY], X[RY], G[RY];
        if (TV) {
#pragma unroll
            for (int q = 0; q <= RY; ++q) Q2[q] = io.ld(a.q[1] + pt, xo, rowoff(q));
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (TV) {
                Q1[r] = io.ld(a.q[0] + pt, xo, rowoff(r + 1));
                if (ND == 3) Q3[r] = io.ld(a.q[ND - 1] + pt, xo, rowoff(r + 1));
            }
            X[r] = io.ld(a.x + pt, xo, rowoff(r + 1));
            G[r] = io.ld(a.g + pt, xo, rowoff(r + 1));
        }

        float Xn[RY], Xb[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            float div = 0.0f;
            if (TV) {
                const bool y_prev = y0 + r > 0;
                // B_d(a)[i] = a[i] - a[i - e_d], a[i] itself on the first index of the axis
                const float l = wave_prev(Q1[r]);
                div = (x_prev ? Q1[r] - l : Q1[r]) + (y_prev ? Q2[r + 1] - Q2[r] : Q2[r + 1]);
                if (ND == 3) {
                    div = div + (z_prev ? Q3[r] - Zp[r] : Q3[r]);
                    Zp[r] = Q3[r];
                }
            }
            float xn = X[r] - a.tau * (G[r] - div);
            if (a.nonneg) xn = xn < 0.0f ? 0.0f : xn;
            Xn[r] = xn;
            Xb[r] = (xn + xn) - X[r];
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) {
                io.st(a.x + pt, xo, rowoff(r + 1), Xn[r]);
                io.st(a.xb + pt, xo, rowoff(r + 1), Xb[r]);
            }
        }
    }
}

// The only launch sites of the two marches: TGV's tile, 4 rows per lane, 2 x 2 waves, 63 columns per wave.
template <int ND, bool ANISO>
static int pdhg_dual_launch(const PdhgArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "PDHG", a.dx, a.dy, a.dz, 63, 2, 2, 4, ND == 3)) return rc;
    pdhg_dual_kernel<ND, ANISO, 4, 2, 2><<<(unsigned)g.blocks, 64 * 2 * 2, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}

template <int ND, bool TV>
static int pdhg_primal_launch(const PdhgArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "PDHG", a.dx, a.dy, a.dz, 63, 2, 2, 4, ND == 3)) return rc;
    pdhg_primal_kernel<ND, TV, 4, 2, 2><<<(unsigned)g.blocks, 64 * 2 * 2, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}

static bool positive_finite(float v) { return v > 0.0f && std::isfinite(v); }

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_pdhg_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    return (size_t)(2 + nd) * work_array_bytes((size_t)dx * dy * dz);   // x-bar, g, q_1..q_nd
}

extern "C" int tomo_pdhg_sino_dual(float *y_dev, const float *r_dev, const float *b_dev, size_t count, int fidelity,
                                   float sigma, void *stream)
{
    TOMO_REQUIRE(fidelity == TOMO_PDHG_LS || fidelity == TOMO_PDHG_L1 || fidelity == TOMO_PDHG_KL,
                 "PDHG: the data term must be TOMO_PDHG_LS, TOMO_PDHG_L1 or TOMO_PDHG_KL");
    TOMO_REQUIRE(positive_finite(sigma), "PDHG: the step size sigma must be positive");
    TOMO_REQUIRE(y_dev && r_dev && b_dev, "NULL data pointer");
    TOMO_REQUIRE(y_dev != r_dev && y_dev != b_dev, "PDHG: the dual array must not alias an array the launch reads");
    if (count == 0) return TOMO_OK;
    hipStream_t st = as_stream(stream);
    if (fidelity == TOMO_PDHG_LS) pdhg_sino_launch<TOMO_PDHG_LS>(y_dev, r_dev, b_dev, count, sigma, st);
    else if (fidelity == TOMO_PDHG_L1) pdhg_sino_launch<TOMO_PDHG_L1>(y_dev, r_dev, b_dev, count, sigma, st);
    else pdhg_sino_launch<TOMO_PDHG_KL>(y_dev, r_dev, b_dev, count, sigma, st);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

// the checks the two marches share; `dz` becomes 1 for nd = 2
#define PDHG_REQUIRE_VOLUME()                                                                                              \
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");                                        \
    TOMO_REQUIRE(nd == 2 || nd == 3, "2D or 3D arrays must be provided only");                                             \
    if (nd == 2) dz = 1;                                                                                                   \
    TOMO_REQUIRE(dx >= 1 && dy >= 1 && dz >= 1, "PDHG needs every dimension >= 1");                                        \
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29),                                                              \
                 "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy)

extern "C" int tomo_pdhg_tv_dual(int device, const float *xbar_dev, float *q1_dev, float *q2_dev, float *q3_dev, int dx,
                                 int dy, int dz, int nd, float sigma, float lambda, int methodTV, void *stream)
{
    PDHG_REQUIRE_VOLUME();
    TOMO_REQUIRE(methodTV == 0 || methodTV == 1, "PDHG: methodTV must be 0 (isotropic) or 1 (anisotropic)");
    TOMO_REQUIRE(positive_finite(sigma), "PDHG: the step size sigma must be positive");
    TOMO_REQUIRE(positive_finite(lambda), "PDHG: lambda must be positive");
    TOMO_REQUIRE(xbar_dev && q1_dev && q2_dev && (nd == 2 || q3_dev), "NULL data pointer");
    TOMO_REQUIRE(q1_dev != xbar_dev && q2_dev != xbar_dev && q3_dev != xbar_dev && q1_dev != q2_dev && q1_dev != q3_dev &&
                 q2_dev != q3_dev, "PDHG: the dual fields must not alias each other or x-bar");
    TOMO_ON_DEVICE(device);
    PdhgArgs a{};
    a.xb = const_cast<float *>(xbar_dev);   // read only in this launch
    a.q[0] = q1_dev; a.q[1] = q2_dev; a.q[2] = nd == 3 ? q3_dev : nullptr;
    a.dx = dx; a.dy = dy; a.dz = dz;
    a.sigma = sigma; a.lambda = lambda;
    hipStream_t st = as_stream(stream);
    const int rc = nd == 3 ? (methodTV ? pdhg_dual_launch<3, true>(a, st) : pdhg_dual_launch<3, false>(a, st))
                           : (methodTV ? pdhg_dual_launch<2, true>(a, st) : pdhg_dual_launch<2, false>(a, st));
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

extern "C" int tomo_pdhg_primal(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *q1_dev,
                                const float *q2_dev, const float *q3_dev, int dx, int dy, int dz, int nd, float tau,
                                int nonneg, void *stream)
{
    PDHG_REQUIRE_VOLUME();
    TOMO_REQUIRE(positive_finite(tau), "PDHG: the step size tau must be positive");
    TOMO_REQUIRE(x_dev && xbar_dev && g_dev, "NULL data pointer");
    const bool tv = q1_dev != nullptr;
    TOMO_REQUIRE(tv ? (q2_dev && (nd == 2 || q3_dev)) : (!q2_dev && !q3_dev),
                 "PDHG: give every dual field of the TV block (q3 for nd = 3 only) or none");
    TOMO_REQUIRE(x_dev != xbar_dev && g_dev != x_dev && g_dev != xbar_dev, "PDHG: x, x-bar and g must not alias");
    for (const float *q : {q1_dev, q2_dev, q3_dev})
        TOMO_REQUIRE(!q || (q != x_dev && q != xbar_dev), "PDHG: a dual field must not alias an array the launch writes");
    TOMO_ON_DEVICE(device);
    PdhgArgs a{};
    a.x = x_dev; a.xb = xbar_dev; a.g = g_dev;
    a.q[0] = const_cast<float *>(q1_dev); a.q[1] = const_cast<float *>(q2_dev);   // read only in this launch
    a.q[2] = nd == 3 ? const_cast<float *>(q3_dev) : nullptr;
    a.dx = dx; a.dy = dy; a.dz = dz;
    a.tau = tau; a.nonneg = nonneg ? 1 : 0;
    hipStream_t st = as_stream(stream);
    const int rc = nd == 3 ? (tv ? pdhg_primal_launch<3, true>(a, st) : pdhg_primal_launch<3, false>(a, st))
                           : (tv ? pdhg_primal_launch<2, true>(a, st) : pdhg_primal_launch<2, false>(a, st));
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}
