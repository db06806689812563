// The four launches SPDHG (stochastic primal-dual hybrid gradient over ordered subsets; Chambolle, Ehrhardt, Richtarik,
// Schoenlieb 2018) adds to the per-subset forward projector and the subset form of the matched back projector for gfx950.
// One block update touches one subset of angles or the TV block.  There is no reference implementation in the tree: what is
// computed is the algorithm stated in docs/kernels/spdhg.md, formula-level parity, unpinned -- tests/_spdhg_oracle.py
// restates it in numpy and the kernels reproduce its float32 form bit for bit (one rounding per operation in the stated
// order, no FMA contraction: -ffp-contract=off and no fmaf here; sqrtf and / are the compiler's correctly rounded ones).
//
//   spdhg_sino_kernel       subset step 2: v = PDHG's sinogram dual on (y_j, r, b_j); d = v - y_j over r, y_j <- v
//   spdhg_primal_kernel     subset step 4: z' = z + delta, zb = z' + w delta, x' = x - tau zb [clamped]; x <- x', z <- z'
//   spdhg_tv_dual_kernel    TV step 1:     p_d = PDHG's projection of q_d + sigma F_d(x); e_d = p_d - q_d, q_d <- p_d
//   spdhg_tv_primal_kernel  TV steps 2, 3: div = sum B_d(e_d); z' = z - div, zb = z' - w div, x' = x - tau zb [clamped]
// The first two are grid-stride streaming kernels (20 B per sample / voxel), the last two plane marches on the skeleton of
// pdhg_kernels.hip (4 rows per lane, 2 x 2 waves, 63 columns per wave; the wave shifts, the plane I/O, the z-march grid and
// the array skew are the one copy in zmarch_common.h): 4 + 3 x 12 = 40 B and 3 x 4 + 16 = 28 B per voxel in 3D.  Neither
// march reads a neighbour of a field it writes, so nothing is ping-ponged.  The element-wise formulas of PDHG's steps 2 and
// 4 are restated here and not shared with pdhg_kernels.hip, whose entries stay as they are.
#include "zmarch_common.h"
#include <initializer_list>

namespace {

// ------------------------------------------------------------------------------------------ subset step 2: the sinogram dual
// PDHG's step 2 (pdhg_sino_one of pdhg_kernels.hip): the prox of the conjugate of the data term at y + sigma r
template <int MODE>
__device__ __forceinline__ float spdhg_sino_prox(float y, float r, float b, float sigma, float one_sigma, float c4)
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

// y <- v and r <- d = v - y
template <int MODE>
__device__ __forceinline__ void spdhg_sino_one(float &y, float &r, float b, float sigma, float one_sigma, float c4)
{
    const float v = spdhg_sino_prox<MODE>(y, r, b, sigma, one_sigma, c4);
    r = v - y;
    y = v;
}

constexpr int STREAM_BLOCK = 256;
constexpr int STREAM_MAX_GRID = 256 * 8;   // 256 CUs x 8 blocks, grid-stride beyond

static unsigned stream_grid(size_t n, bool vec)
{
    const size_t items = vec ? (n >> 2) : n;
    size_t grid = (items + STREAM_BLOCK - 1) / STREAM_BLOCK;
    if (grid < 1) grid = 1;
    if (grid > (size_t)STREAM_MAX_GRID) grid = STREAM_MAX_GRID;
    return (unsigned)grid;
}

static bool aligned16(const void *a, const void *b, const void *c)
{
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15u) == 0;
}

// VEC: 16-byte accesses over the first n / 4 quads and a scalar tail by block 0 (all three arrays 16-byte aligned)
template <int MODE, bool VEC>
__global__ __launch_bounds__(STREAM_BLOCK) void spdhg_sino_kernel(float *y, float *r, const float *b, size_t n, float sigma,
                                                                  float one_sigma, float c4)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const size_t n4 = n >> 2;
        for (size_t i = first; i < n4; i += stride) {
            float4 vy = reinterpret_cast<const float4 *>(y)[i];
            float4 vr = reinterpret_cast<const float4 *>(r)[i];
            const float4 vb = reinterpret_cast<const float4 *>(b)[i];
            spdhg_sino_one<MODE>(vy.x, vr.x, vb.x, sigma, one_sigma, c4);
            spdhg_sino_one<MODE>(vy.y, vr.y, vb.y, sigma, one_sigma, c4);
            spdhg_sino_one<MODE>(vy.z, vr.z, vb.z, sigma, one_sigma, c4);
            spdhg_sino_one<MODE>(vy.w, vr.w, vb.w, sigma, one_sigma, c4);
            reinterpret_cast<float4 *>(y)[i] = vy;
            reinterpret_cast<float4 *>(r)[i] = vr;
        }
        const size_t i = (n4 << 2) + threadIdx.x;
        if (blockIdx.x == 0 && i < n) {
            float sy = y[i], sr = r[i];
            spdhg_sino_one<MODE>(sy, sr, b[i], sigma, one_sigma, c4);
            y[i] = sy;
            r[i] = sr;
        }
    } else {
        for (size_t i = first; i < n; i += stride) {
            float sy = y[i], sr = r[i];
            spdhg_sino_one<MODE>(sy, sr, b[i], sigma, one_sigma, c4);
            y[i] = sy;
            r[i] = sr;
        }
    }
}

template <int MODE>
static void spdhg_sino_launch(float *y, float *r, const float *b, size_t n, float sigma, hipStream_t st)
{
    const bool vec = aligned16(y, r, b);
    const float one_sigma = 1.0f + sigma, c4 = 4.0f * sigma;
    if (vec)
        spdhg_sino_kernel<MODE, true><<<stream_grid(n, true), STREAM_BLOCK, 0, st>>>(y, r, b, n, sigma, one_sigma, c4);
    else
        spdhg_sino_kernel<MODE, false><<<stream_grid(n, false), STREAM_BLOCK, 0, st>>>(y, r, b, n, sigma, one_sigma, c4);
}

// ------------------------------------------------------------------------------------------ subset step 4: the primal
__device__ __forceinline__ void spdhg_primal_one(float &x, float &z, float delta, float tau, float w, int nonneg)
{
    const float zn = z + delta;
    const float zb = zn + w * delta;
    float xn = x - tau * zb;
    if (nonneg) xn = xn < 0.0f ? 0.0f : xn;
    x = xn;
    z = zn;
}

template <bool VEC>
__global__ __launch_bounds__(STREAM_BLOCK) void spdhg_primal_kernel(float *x, float *z, const float *delta, size_t n, float tau,
                                                                    float w, int nonneg)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const size_t n4 = n >> 2;
        for (size_t i = first; i < n4; i += stride) {
            float4 vx = reinterpret_cast<const float4 *>(x)[i];
            float4 vz = reinterpret_cast<const float4 *>(z)[i];
            const float4 vd = reinterpret_cast<const float4 *>(delta)[i];
            spdhg_primal_one(vx.x, vz.x, vd.x, tau, w, nonneg);
            spdhg_primal_one(vx.y, vz.y, vd.y, tau, w, nonneg);
            spdhg_primal_one(vx.z, vz.z, vd.z, tau, w, nonneg);
            spdhg_primal_one(vx.w, vz.w, vd.w, tau, w, nonneg);
            reinterpret_cast<float4 *>(x)[i] = vx;
            reinterpret_cast<float4 *>(z)[i] = vz;
        }
        const size_t i = (n4 << 2) + threadIdx.x;
        if (blockIdx.x == 0 && i < n) {
            float sx = x[i], sz = z[i];
            spdhg_primal_one(sx, sz, delta[i], tau, w, nonneg);
            x[i] = sx;
            z[i] = sz;
        }
    } else {
        for (size_t i = first; i < n; i += stride) {
            float sx = x[i], sz = z[i];
            spdhg_primal_one(sx, sz, delta[i], tau, w, nonneg);
            x[i] = sx;
            z[i] = sz;
        }
    }
}

// ------------------------------------------------------------------------------------------ the TV update
struct SpdhgArgs {
    float *x, *z;      // the primal variable and z = sum K_j^T y_j
    float *q[3];       // the TV dual
    float *e[3];       // its change p - q of this update
    int dx, dy, dz;
    float sigma, tau, w, lambda;
    int nonneg;
};

// TV step 1.  A lane owns RY rows of one x column and walks z.  The +x neighbour is the next lane (lane 63 of a wave is a
// halo lane: 63 columns per wave), the +y neighbour the next register (one halo row below the tile), the +z neighbour the
// plane loaded one step ahead, which becomes the current plane of the next step: x is read once per launch (plus halos),
// q read and written once, e written once.
template <int ND, bool ANISO, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void spdhg_tv_dual_kernel(SpdhgArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
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
    for (int q = 0; q <= RY; ++q) cur[q] = io.ld(a.x + sz * zc0, xo, rowoff(q));

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_next = t < dz - 1;
        if (ND == 3) {
            const size_t pn = sz * min(t + 1, dz - 1);
#pragma unroll
            for (int q = 0; q <= RY; ++q) nxt[q] = io.ld(a.x + pn, xo, rowoff(q));
        }
        float Q[ND][RY], E[ND][RY];
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int r = 0; r < RY; ++r) Q[d][r] = io.ld(a.q[d] + sz * t, xo, rowoff(r));

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_next = y0 + r < dy - 1;
            // F_d(x): a[i + e_d] - a[i], exactly 0 on the last index of the axis
            const float c = cur[r];
            const float cx = wave_next(c);
            float F[3];
            F[0] = x_next ? cx - c : 0.0f;
            F[1] = y_next ? cur[r + 1] - c : 0.0f;
            F[2] = (ND == 3 && z_next) ? nxt[r] - c : 0.0f;
            float P[ND];
#pragma unroll
            for (int d = 0; d < ND; ++d) P[d] = Q[d][r] + a.sigma * F[d];
            if (ANISO) {
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    const float v = P[d] < -a.lambda ? -a.lambda : P[d];
                    P[d] = v > a.lambda ? a.lambda : v;
                }
            } else {
                float m = P[0] * P[0] + P[1] * P[1];
                if (ND == 3) m = m + P[ND - 1] * P[ND - 1];
                const float n = sqrtf(m) / a.lambda;
                const float den = n > 1.0f ? n : 1.0f;   // p / 1 is p: the same bits as leaving it alone
#pragma unroll
                for (int d = 0; d < ND; ++d) P[d] = P[d] / den;
            }
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                E[d][r] = P[d] - Q[d][r];
                Q[d][r] = P[d];
            }
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) {
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    io.st(a.q[d] + sz * t, xo, rowoff(r), Q[d][r]);
                    io.st(a.e[d] + sz * t, xo, rowoff(r), E[d][r]);
                }
            }
        }
        if (ND == 3) {
#pragma unroll
            for (int q = 0; q <= RY; ++q) cur[q] = nxt[q];
        }
    }
}

// TV steps 2 and 3.  The mirror image: the -x neighbour is the previous lane (lane 0 of a wave is the halo lane), the -y
// neighbour the previous register (one halo row above the tile, e2 only), the -z neighbour the carried registers of the
// plane before (e3; a z-chunk loads them once for the plane below its first).  e is read and not written; x and z are read
// and written at the lane's own voxels only.
template <int ND, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void spdhg_tv_primal_kernel(SpdhgArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
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

    // the plane below: e3
    float Zp[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) Zp[r] = 0.0f;
    if (ND == 3 && zc0 > 0) {
#pragma unroll
        for (int r = 0; r < RY; ++r) Zp[r] = io.ld(a.e[ND - 1] + sz * (zc0 - 1), xo, rowoff(r + 1));
    }

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_prev = t > 0;
        const size_t pt = sz * t;
        float E1[RY], E2[RY + 1], E3[RY], X[RY], Z[RY];
#pragma unroll
        for (int q = 0; q <= RY; ++q) E2[q] = io.ld(a.e[1] + pt, xo, rowoff(q));
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            E1[r] = io.ld(a.e[0] + pt, xo, rowoff(r + 1));
            if (ND == 3) E3[r] = io.ld(a.e[ND - 1] + pt, xo, rowoff(r + 1));
            X[r] = io.ld(a.x + pt, xo, rowoff(r + 1));
            Z[r] = io.ld(a.z + pt, xo, rowoff(r + 1));
        }

        float Xn[RY], Zn[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_prev = y0 + r > 0;
            // B_d(a)[i] = a[i] - a[i - e_d], a[i] itself on the first index of the axis
            const float l = wave_prev(E1[r]);
            float div = (x_prev ? E1[r] - l : E1[r]) + (y_prev ? E2[r + 1] - E2[r] : E2[r + 1]);
            if (ND == 3) {
                div = div + (z_prev ? E3[r] - Zp[r] : E3[r]);
                Zp[r] = E3[r];
            }
            const float zn = Z[r] - div;
            const float zb = zn - a.w * div;
            float xn = X[r] - a.tau * zb;
            if (a.nonneg) xn = xn < 0.0f ? 0.0f : xn;
            Xn[r] = xn;
            Zn[r] = zn;
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) {
                io.st(a.x + pt, xo, rowoff(r + 1), Xn[r]);
                io.st(a.z + pt, xo, rowoff(r + 1), Zn[r]);
            }
        }
    }
}

// The only launch sites of the two marches: the tile of the PDHG marches, 4 rows per lane, 2 x 2 waves, 63 columns per wave.
template <int ND, bool ANISO>
static int spdhg_tv_dual_launch(const SpdhgArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "SPDHG", a.dx, a.dy, a.dz, 63, 2, 2, 4, ND == 3)) return rc;
    spdhg_tv_dual_kernel<ND, ANISO, 4, 2, 2><<<(unsigned)g.blocks, 64 * 2 * 2, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}

template <int ND>
static int spdhg_tv_primal_launch(const SpdhgArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "SPDHG", a.dx, a.dy, a.dz, 63, 2, 2, 4, ND == 3)) return rc;
    spdhg_tv_primal_kernel<ND, 4, 2, 2><<<(unsigned)g.blocks, 64 * 2 * 2, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}

static bool positive_finite(float v) { return v > 0.0f && std::isfinite(v); }

// no two of the pointers are equal (null pointers excepted)
static bool distinct(std::initializer_list<const float *> ptrs)
{
    for (auto i = ptrs.begin(); i != ptrs.end(); ++i)
        for (auto k = i + 1; k != ptrs.end(); ++k)
            if (*i && *i == *k) return false;
    return true;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_spdhg_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    return (size_t)(2 + 2 * nd) * work_array_bytes((size_t)dx * dy * dz);   // z, delta, q_1..q_nd, e_1..e_nd
}

extern "C" int tomo_spdhg_sino_dual(float *y_dev, float *r_dev, const float *b_dev, size_t count, int fidelity, float sigma,
                                    void *stream)
{
    TOMO_REQUIRE(fidelity == TOMO_PDHG_LS || fidelity == TOMO_PDHG_L1 || fidelity == TOMO_PDHG_KL,
                 "SPDHG: the data term must be TOMO_PDHG_LS, TOMO_PDHG_L1 or TOMO_PDHG_KL");
    TOMO_REQUIRE(positive_finite(sigma), "SPDHG: the step size sigma must be positive");
    TOMO_REQUIRE(y_dev && r_dev && b_dev, "NULL data pointer");
    TOMO_REQUIRE(distinct({y_dev, r_dev, b_dev}), "SPDHG: the dual array, the projection and the data must not alias");
    if (count == 0) return TOMO_OK;
    hipStream_t st = as_stream(stream);
    if (fidelity == TOMO_PDHG_LS) spdhg_sino_launch<TOMO_PDHG_LS>(y_dev, r_dev, b_dev, count, sigma, st);
    else if (fidelity == TOMO_PDHG_L1) spdhg_sino_launch<TOMO_PDHG_L1>(y_dev, r_dev, b_dev, count, sigma, st);
    else spdhg_sino_launch<TOMO_PDHG_KL>(y_dev, r_dev, b_dev, count, sigma, st);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

extern "C" int tomo_spdhg_primal(float *x_dev, float *z_dev, const float *delta_dev, size_t count, float tau, float w,
                                 int nonneg, void *stream)
{
    TOMO_REQUIRE(positive_finite(tau), "SPDHG: the step size tau must be positive");
    TOMO_REQUIRE(positive_finite(w), "SPDHG: the extrapolation weight w (1 / the block's probability) must be positive");
    TOMO_REQUIRE(x_dev && z_dev && delta_dev, "NULL data pointer");
    TOMO_REQUIRE(distinct({x_dev, z_dev, delta_dev}), "SPDHG: x, z and delta must not alias");
    if (count == 0) return TOMO_OK;
    hipStream_t st = as_stream(stream);
    if (aligned16(x_dev, z_dev, delta_dev))
        spdhg_primal_kernel<true><<<stream_grid(count, true), STREAM_BLOCK, 0, st>>>(x_dev, z_dev, delta_dev, count, tau, w, nonneg ? 1 : 0);
    else
        spdhg_primal_kernel<false><<<stream_grid(count, false), STREAM_BLOCK, 0, st>>>(x_dev, z_dev, delta_dev, count, tau, w, nonneg ? 1 : 0);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

// the checks the two marches share; `dz` becomes 1 for nd = 2
#define SPDHG_REQUIRE_VOLUME()                                                                                             \
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");                                        \
    TOMO_REQUIRE(nd == 2 || nd == 3, "2D or 3D arrays must be provided only");                                             \
    if (nd == 2) dz = 1;                                                                                                   \
    TOMO_REQUIRE(dx >= 1 && dy >= 1 && dz >= 1, "SPDHG needs every dimension >= 1");                                       \
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29),                                                              \
                 "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy)

extern "C" int tomo_spdhg_tv_dual(int device, const float *x_dev, float *q1_dev, float *q2_dev, float *q3_dev, float *e1_dev,
                                  float *e2_dev, float *e3_dev, int dx, int dy, int dz, int nd, float sigma, float lambda,
                                  int methodTV, void *stream)
{
    SPDHG_REQUIRE_VOLUME();
    TOMO_REQUIRE(methodTV == 0 || methodTV == 1, "SPDHG: methodTV must be 0 (isotropic) or 1 (anisotropic)");
    TOMO_REQUIRE(positive_finite(sigma), "SPDHG: the step size sigma must be positive");
    TOMO_REQUIRE(positive_finite(lambda), "SPDHG: lambda must be positive");
    TOMO_REQUIRE(x_dev && q1_dev && q2_dev && e1_dev && e2_dev && (nd == 2 || (q3_dev && e3_dev)), "NULL data pointer");
    if (nd == 2) q3_dev = e3_dev = nullptr;
    TOMO_REQUIRE(distinct({x_dev, q1_dev, q2_dev, q3_dev, e1_dev, e2_dev, e3_dev}),
                 "SPDHG: the dual fields and their changes must not alias each other or x");
    TOMO_ON_DEVICE(device);
    SpdhgArgs a{};
    a.x = const_cast<float *>(x_dev);   // read only in this launch
    a.q[0] = q1_dev; a.q[1] = q2_dev; a.q[2] = q3_dev;
    a.e[0] = e1_dev; a.e[1] = e2_dev; a.e[2] = e3_dev;
    a.dx = dx; a.dy = dy; a.dz = dz;
    a.sigma = sigma; a.lambda = lambda;
    hipStream_t st = as_stream(stream);
    const int rc = nd == 3 ? (methodTV ? spdhg_tv_dual_launch<3, true>(a, st) : spdhg_tv_dual_launch<3, false>(a, st))
                           : (methodTV ? spdhg_tv_dual_launch<2, true>(a, st) : spdhg_tv_dual_launch<2, false>(a, st));
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

extern "C" int tomo_spdhg_tv_primal(int device, float *x_dev, float *z_dev, const float *e1_dev, const float *e2_dev,
                                    const float *e3_dev, int dx, int dy, int dz, int nd, float tau, float w, int nonneg,
                                    void *stream)
{
    SPDHG_REQUIRE_VOLUME();
    TOMO_REQUIRE(positive_finite(tau), "SPDHG: the step size tau must be positive");
    TOMO_REQUIRE(positive_finite(w), "SPDHG: the extrapolation weight w (1 / the block's probability) must be positive");
    TOMO_REQUIRE(x_dev && z_dev && e1_dev && e2_dev && (nd == 2 || e3_dev), "NULL data pointer");
    if (nd == 2) e3_dev = nullptr;
    TOMO_REQUIRE(distinct({x_dev, z_dev, e1_dev, e2_dev, e3_dev}), "SPDHG: x, z and the changes of the dual fields must not alias");
    TOMO_ON_DEVICE(device);
    SpdhgArgs a{};
    a.x = x_dev; a.z = z_dev;
    a.e[0] = const_cast<float *>(e1_dev); a.e[1] = const_cast<float *>(e2_dev);   // read only in this launch
    a.e[2] = const_cast<float *>(e3_dev);
    a.dx = dx; a.dy = dy; a.dz = dz;
    a.tau = tau; a.w = w; a.nonneg = nonneg ? 1 : 0;
    hipStream_t st = as_stream(stream);
    const int rc = nd == 3 ? spdhg_tv_primal_launch<3>(a, st) : spdhg_tv_primal_launch<2>(a, st);
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}
