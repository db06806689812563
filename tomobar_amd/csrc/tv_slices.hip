// Slice-wise PD_TV and ROF_TV for gfx950: the 2D total variation of every (y, x) slice of a stack [nslices][dy][dx], all
// slices in one launch (docs/kernels/slicewise.md).  What a slice receives is exactly what tomo_pdtv / tomo_roftv with
// nd = 2 return for it: the same iteration, the same roundings, no coupling along the slice axis.
//
// tv_kernels.hip and its .inl files are pinned by hash (profiles/pmc_traffic.json is keyed to their bytes; see
// zmarch_common.h), so nothing is shared with them at source level.  The per-pixel arithmetic below -- the dual step, the
// projection, the primal step, the binary16 round trip, ROF's minmod, double-precision sum and FMA-corrected roundings --
// is copied OPERATION FOR OPERATION from the 2D forms there (pd_dual_t / pd_primal_t / mk_sqrt / mk_recip / DualIO of
// tv_kernels.hip, pd_rows2d.inl, rof_mm / rof_eval FAST = 3 / the ND = 2 step of rof_zmarch.inl); do not "simplify" an
// expression here: tests/test_gpu_slicewise.py holds the copies to the originals bit for bit.
//   * PD_TV: pd_slices_kernel, the batched form of pd_rows2d: a wave owns a tile of RY rows x (64 - 2K) columns of ONE
//     slice and runs K <= 3 iterations per pass with the tile and its K-deep halo in registers.  The tile index decodes
//     to (slice, tile row, tile column); buffer descriptors are per (array, slice).
//   * ROF_TV: rof_slices_kernel, one launch per iteration over all slices, D1 / D2 in registers.
// Variants: g_variant_pdtv 0 (relaxed float32 arithmetic for float32 duals, the reference's roundings for binary16 duals)
// and 22 (the reference's roundings for both), g_variant_roftv 0, as the 2D path; the dev-only variants have no
// slice-wise form.
#include "zmarch_common.h"   // wave_prev / wave_next, align_up, WORK_SKEW, the early-stopping rule, march_run
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------ copied arithmetic
// binary16 rounding of a float32 RESULT (f32_to_half_twice_rounded of tv_kernels.hip): the empty asm keeps the compiler
// from folding "fmaf then float->half" into one v_fma_mixlo_f16, which would round once where the reference rounds twice
__device__ __forceinline__ __half f32_to_half_twice_rounded(float v)
{
    asm volatile("" : "+v"(v));
    return __float2half_rn(v);
}
template <typename T> struct DualRt;
template <> struct DualRt<float> {
    static __device__ __forceinline__ float rt(float v) { return v; }
};
template <> struct DualRt<__half> {
    static __device__ __forceinline__ float rt(float v) { return __half2float(f32_to_half_twice_rounded(v)); }
};

// mk_sqrt / mk_recip of tv_kernels.hip: sqrtf(x) and 1.0f / q correctly rounded through FMA correction steps
__device__ __forceinline__ float mk_sqrt(float x)
{
    const float r = __builtin_amdgcn_rsqf(x);
    float q = x * r, h = 0.5f * r;
    const float e = fmaf(-h, q, 0.5f);
    q = fmaf(q, e, q);
    h = fmaf(h, e, h);
    return fmaf(fmaf(-q, q, x), h, q);
}
__device__ __forceinline__ float mk_recip(float q)
{
    const float y = __builtin_amdgcn_rcpf(q);
    return fmaf(fmaf(-q, y, 1.0f), y, y);
}

// pd_dual_t<ANISO, FAST, 2> of tv_kernels.hip, FAST = 1 (relaxed) and 2 (the reference's roundings): dual ascent and the
// projection onto the unit ball (isotropic) / unit square (anisotropic)
template <bool ANISO, int FAST>
__device__ __forceinline__ void pd_dual2(float (&p)[2], const float (&g)[2], float sigma)
{
#pragma unroll
    for (int c = 0; c < 2; ++c) p[c] = fmaf(sigma, g[c], p[c]);
    if (!ANISO) {
        float nrm = p[0] * p[0];
        nrm = fmaf(p[1], p[1], nrm);
        if (FAST == 2) {
            const float r = mk_recip(mk_sqrt(nrm));
            const float rr = nrm > 1.0f ? r : 1.0f;
#pragma unroll
            for (int c = 0; c < 2; ++c) p[c] *= rr;
        } else {
            const float r = nrm > 1.0f ? __builtin_amdgcn_rsqf(nrm) : 1.0f;
#pragma unroll
            for (int c = 0; c < 2; ++c) p[c] *= r;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 2; ++c)
            p[c] = fabsf(p[c]) > 1.0f ? copysignf(1.0f, p[c]) : p[c];
    }
}

// pd_primal_t<FAST> of tv_kernels.hip, FAST = 1 / 2 (inv1lt = RN(1 / (1 + lt)), formed on the host)
template <int FAST>
__device__ __forceinline__ float pd_primal2(float u_in, float input, float div, float tau, float lt, float inv1lt, float theta,
                                            bool nonneg)
{
    const float u = (nonneg && u_in < 0.0f) ? 0.0f : u_in;
    float t = fmaf(-tau, div, u);
    t = fmaf(lt, input, t);
    float nu = t * inv1lt;
    if (FAST == 2) nu = fmaf(fmaf(-(1.0f + lt), nu, t), inv1lt, nu);
    return fmaf(theta, nu - u, nu);
}

// rof_mm of tv_kernels.hip: (0.5 (sign(n1) + sign(n0)) min(|n1|, |n0|))^2
__device__ __forceinline__ float rof_mm(float n0, float n1)
{
    const float m = fmaxf(fmaxf(fminf(n1, n0), fminf(-n1, -n0)), 0.0f);
    return m * m;
}

// nrm of rof_eval (rof_zmarch.inl), FAST = 3: nom / sqrt((double)((d1 + d2) + d3) + 1e-8) with the reference's roundings
__device__ __forceinline__ float rof_nrm(float nom, float d1, float d2, float d3)
{
    const float x = (float)((double)((d1 + d2) + d3) + 1.0e-8);
    const float r = __builtin_amdgcn_rsqf(x);
    float q = x * r, h = 0.5f * r;
    const float e = fmaf(-h, q, 0.5f);
    q = fmaf(q, e, q);
    h = fmaf(h, e, h);
    q = fmaf(fmaf(-q, q, x), h, q);
    float y = __builtin_amdgcn_rcpf(q);
    y = fmaf(fmaf(-q, y, 1.0f), y, y);
    float z = nom * y;
    z = fmaf(fmaf(-q, z, nom), y, z);
    return z;
}

// ------------------------------------------------------------------------------------------ addressing
// One buffer descriptor per (array, slice): base = the slice's first element, num_records = the slice's bytes, so a
// descriptor stays under 2 GiB whatever nslices is.  `xo` is the FLOAT byte offset of the lane's (clamped) column inside
// a row, `ro` the FLOAT byte offset of the (clamped) row inside the slice (wave-uniform, the instruction's soffset):
// xo + ro always lies inside the slice.  binary16 arrays halve both.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slice_rs(const void *slice, int nbytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)slice, 0, nbytes, 0x00020000);
}
__device__ __forceinline__ float ld_f(__amdgpu_buffer_rsrc_t r, unsigned xo, int ro)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)xo, ro, 0));
}
__device__ __forceinline__ void st_f(__amdgpu_buffer_rsrc_t r, unsigned xo, int ro, float v)
{
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, (int)xo, ro, 0);
}
template <typename T> struct DualMem;
template <> struct DualMem<float> {
    static __device__ __forceinline__ __amdgpu_buffer_rsrc_t rs(const void *slice, int fbytes) { return slice_rs(slice, fbytes); }
    static __device__ __forceinline__ float ld(__amdgpu_buffer_rsrc_t r, unsigned xo, int ro) { return ld_f(r, xo, ro); }
    static __device__ __forceinline__ void st(__amdgpu_buffer_rsrc_t r, unsigned xo, int ro, float v) { st_f(r, xo, ro, v); }
};
template <> struct DualMem<__half> {
    static __device__ __forceinline__ __amdgpu_buffer_rsrc_t rs(const void *slice, int fbytes) { return slice_rs(slice, fbytes >> 1); }
    static __device__ __forceinline__ float ld(__amdgpu_buffer_rsrc_t r, unsigned xo, int ro)
    {
        const unsigned short h = __builtin_amdgcn_raw_buffer_load_b16(r, (int)(xo >> 1), ro >> 1, 0);
        return __half2float(__builtin_bit_cast(__half, h));
    }
    static __device__ __forceinline__ void st(__amdgpu_buffer_rsrc_t r, unsigned xo, int ro, float v)
    {
        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, f32_to_half_twice_rounded(v)), r, (int)(xo >> 1), ro >> 1, 0);
    }
};

// The tile a wave owns: workgroups of four waves, wave w of workgroup b takes tile 4 b + w of the slice-major, row-major
// list (slice, tile row, tile column); a workgroup may span two slices, the last one may be partly empty.
struct TileId {
    int slice, xb, yb;
    bool valid;
};
__device__ __forceinline__ TileId tile_of_wave(int gx, int gy, int tiles)
{
    const int tile = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6));
    TileId t;
    t.valid = tile < tiles;  // wave-uniform
    const int per_slice = gx * gy;
    t.slice = tile / per_slice;
    const int q = tile - t.slice * per_slice;
    t.yb = q / gx;
    t.xb = q - t.yb * gx;
    return t;
}

// ------------------------------------------------------------------------------------------ PD_TV
struct PdSliceArgs {
    const float *in;
    const float *u_in;
    float *u_out;
    const void *p_in[2];
    void *p_out[2];
    int dx, dy;
    float sigma, tau, lt, theta, inv1lt;
    int p_in_zero;   // the input duals are all zero (first launch of a prox): do not read them
    int p_out_skip;  // do not store the output duals (last launch of a prox)
};

// pd_rows2d_kernel (pd_rows2d.inl) over a stack of slices.  Iteration s of the launch evaluates the duals on rows
// -(K-s) .. RY+(K-s)-2 and the primal variable on rows -(K-s-1) .. RY+(K-s-1)-1 of the tile (lanes s .. 63-s / s+1 .. 62-s),
// so after K iterations rows 0 .. RY-1 and lanes K .. 63-K hold U^{n+K}, P^{n+K}.  Halo rows / lanes outside the slice are
// loaded from clamped addresses INSIDE THE SAME SLICE; every use of such a value is behind the reference's own edge rule
// (mirror at the far edge, zero "previous" dual at index 0), so neither it nor anything of another slice reaches a
// stored pixel.  No LDS, no barrier.
template <typename T, bool NONNEG, bool ANISO, int FAST, int K, int RY>
__global__ __launch_bounds__(256) void pd_slices_kernel(PdSliceArgs a, int gx, int gy, int tiles)
{
    constexpr int NR = RY + 2 * K;
    const TileId id = tile_of_wave(gx, gy, tiles);
    if (!id.valid) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int dx = a.dx, dy = a.dy;
    const int x = id.xb * (64 - 2 * K) - K + lane;
    const int y0 = id.yb * RY;
    const bool x_last = (x == dx - 1);
    const bool x_has_prev = (x > 0);
    const bool emit_lane = (lane >= K) && (lane <= 63 - K) && (x < dx);
    const unsigned xo = (unsigned)min(max(x, 0), dx - 1) * 4u;
    const int pitch = dx * 4;
    const int fbytes = dx * dy * 4;
    auto rowoff = [&](int i) __attribute__((always_inline)) { return min(max(y0 + i - K, 0), dy - 1) * pitch; };
    const size_t so = (size_t)id.slice * (size_t)dx * (size_t)dy;  // elements before this slice
    const __amdgpu_buffer_rsrc_t r_uin = slice_rs(a.u_in + so, fbytes), r_in = slice_rs(a.in + so, fbytes);

    float U[NR], In[NR], P0[NR], P1[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        U[i] = ld_f(r_uin, xo, rowoff(i));
        In[i] = ld_f(r_in, xo, rowoff(i));
        P0[i] = 0.0f; P1[i] = 0.0f;
    }
    if (!a.p_in_zero) {  // uniform: the first launch of a prox starts from zero duals (nothing to read)
        const __amdgpu_buffer_rsrc_t r_p0 = DualMem<T>::rs((const T *)a.p_in[0] + so, fbytes), r_p1 = DualMem<T>::rs((const T *)a.p_in[1] + so, fbytes);
#pragma unroll
        for (int i = 0; i < NR - 1; ++i) {
            P0[i] = DualMem<T>::ld(r_p0, xo, rowoff(i));
            P1[i] = DualMem<T>::ld(r_p1, xo, rowoff(i));
        }
    }
#pragma unroll
    for (int s = 0; s < K; ++s) {
        // ---- duals of iteration s, rows -(K-s) .. RY+(K-s)-2
#pragma unroll
        for (int r = -(K - s); r <= RY + (K - s) - 2; ++r) {
            const int i = r + K;
            const int y = y0 + r;
            const float u = U[i];
            const float ux = wave_next(u), uxm = wave_prev(u);
            float g[2], p[2];
            g[0] = (x_last ? (x_has_prev ? uxm : 0.0f) : ux) - u;           // forward difference, mirrored at the far edge
            g[1] = ((y == dy - 1) ? ((y > 0) ? U[i > 0 ? i - 1 : 0] : 0.0f) : U[i + 1]) - u;
            p[0] = P0[i]; p[1] = P1[i];
            pd_dual2<ANISO, FAST>(p, g, a.sigma);
            P0[i] = p[0]; P1[i] = p[1];
        }
        // ---- primal variable of iteration s, rows -(K-s-1) .. RY+(K-s-1)-1 (descending: row i reads the dual of row i-1)
#pragma unroll
        for (int r = RY + (K - s - 1) - 1; r >= -(K - s - 1); --r) {
            const int i = r + K;
            const int y = y0 + r;
            const float p0l = wave_prev(P0[i]);
            const float px = x_has_prev ? p0l : 0.0f;
            const float py = (y > 0) ? P1[i - 1] : 0.0f;
            const float div = (-(P0[i] - px)) + (-(P1[i] - py));
            U[i] = pd_primal2<FAST>(U[i], In[i], div, a.tau, a.lt, a.inv1lt, a.theta, NONNEG);
        }
        if (sizeof(T) == 2 && s + 1 < K) {  // what the next iteration reads back is the stored binary16 value
#pragma unroll
            for (int i = 0; i < NR; ++i) { P0[i] = DualRt<T>::rt(P0[i]); P1[i] = DualRt<T>::rt(P1[i]); }
        }
    }
    if (!emit_lane) return;
    const __amdgpu_buffer_rsrc_t r_u = slice_rs(a.u_out + so, fbytes);
    const __amdgpu_buffer_rsrc_t r_q0 = DualMem<T>::rs((T *)a.p_out[0] + so, fbytes), r_q1 = DualMem<T>::rs((T *)a.p_out[1] + so, fbytes);
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        if (y0 + r < dy) {
            const int ro = (y0 + r) * pitch;
            st_f(r_u, xo, ro, U[r + K]);
            if (!a.p_out_skip) {  // uniform: nobody reads the duals of the last launch of a prox
                DualMem<T>::st(r_q0, xo, ro, P0[r + K]);
                DualMem<T>::st(r_q1, xo, ro, P1[r + K]);
            }
        }
    }
}

constexpr int PD_RY = 8;  // rows per tile: pd_rows2d's (docs/kernels/slicewise.md, "Choices")

// number of tiles of a launch with `tile_x` columns and `ry` rows per wave, or an error
static int slice_tiles(const char *op, int dx, int dy, int nslices, int tile_x, int ry, int &gx, int &gy, int &tiles)
{
    gx = ceil_div(dx, tile_x);
    gy = ceil_div(dy, ry);
    const long n = (long)gx * gy * nslices;
    if (n > 0x7fffffffL - 3) return tomo_fail(TOMO_E_INVALID, "stack too large for one slice-wise %s launch", op);
    tiles = (int)n;
    return TOMO_OK;
}

template <typename T, bool NN, bool AN, int FAST, int K>
static int pd_slices_launch(PdSliceArgs a, int nslices, hipStream_t st)
{
    int gx, gy, tiles;
    if (int rc = slice_tiles("PD_TV", a.dx, a.dy, nslices, 64 - 2 * K, PD_RY, gx, gy, tiles)) return rc;
    a.inv1lt = 1.0f / (1.0f + a.lt);
    pd_slices_kernel<T, NN, AN, FAST, K, PD_RY><<<(unsigned)((tiles + 3) / 4), 256, 0, st>>>(a, gx, gy, tiles);
    return TOMO_OK;
}

template <typename T, bool NN, bool AN, int FAST>
static int pd_slices_launch_k(const PdSliceArgs &a, int nslices, int k, hipStream_t st)
{
    if (k == 3) return pd_slices_launch<T, NN, AN, FAST, 3>(a, nslices, st);
    if (k == 2) return pd_slices_launch<T, NN, AN, FAST, 2>(a, nslices, st);
    return pd_slices_launch<T, NN, AN, FAST, 1>(a, nslices, st);
}

template <typename T> struct type_c { using type = T; };

// run-time flags to template arguments.  The arithmetic level follows pd_arith of tv_kernels.hip: binary16 duals and
// variant 22 run the reference's roundings (FAST = 2), float32 duals of variant 0 the relaxed arithmetic (FAST = 1).
static int pd_slices_dispatch(const PdSliceArgs &a, int nslices, int k, int methodTV, int nonneg, int half, int variant, hipStream_t st)
{
    auto flags = [&](auto t, auto f) -> int {
        using T = typename decltype(t)::type;
        constexpr int F = decltype(f)::value;
        if (nonneg) return methodTV ? pd_slices_launch_k<T, true, true, F>(a, nslices, k, st) : pd_slices_launch_k<T, true, false, F>(a, nslices, k, st);
        return methodTV ? pd_slices_launch_k<T, false, true, F>(a, nslices, k, st) : pd_slices_launch_k<T, false, false, F>(a, nslices, k, st);
    };
    int rc;
    if (half) rc = flags(type_c<__half>{}, std::integral_constant<int, 2>{});
    else if (variant == 22) rc = flags(type_c<float>{}, std::integral_constant<int, 2>{});
    else rc = flags(type_c<float>{}, std::integral_constant<int, 1>{});
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

// ------------------------------------------------------------------------------------------ ROF_TV
struct RofSliceArgs {
    const float *in;
    const float *u_in;
    float *u_out;
    int dx, dy;
    float lambda, tau;
};

// One ROF_TV iteration of every slice: the ND = 2 step of rof_zmarch_kernel (rof_zmarch.inl, its EDGE form: the reflection
// selects on every tile -- the same operands as the interior form reads).  A wave owns RY rows x 60 columns of one slice
// (two halo lanes either side, rows -2 .. RY loaded); D1 / D2 are evaluated once per pixel on rows -1 .. RY-1 and never
// leave the registers: 12 B per pixel and iteration.
template <bool HALF, int RY>
__global__ __launch_bounds__(256) void rof_slices_kernel(RofSliceArgs a, int gx, int gy, int tiles)
{
    const TileId id = tile_of_wave(gx, gy, tiles);
    if (!id.valid) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int dx = a.dx, dy = a.dy;
    const int x = id.xb * 60 - 2 + lane;
    const int y0 = id.yb * RY;
    const bool x_first = (x == 0), x_last = (x == dx - 1);
    const bool emit_lane = (lane >= 2) && (lane <= 61) && (x < dx);
    const unsigned xo = (unsigned)min(max(x, 0), dx - 1) * 4u;
    const int pitch = dx * 4;
    const int fbytes = dx * dy * 4;
    // row slot index q = r + 2 (rows -2 .. RY), clamped into the slice
    auto rowoff = [&](int q) __attribute__((always_inline)) { return min(max(y0 + q - 2, 0), dy - 1) * pitch; };
    const size_t so = (size_t)id.slice * (size_t)dx * (size_t)dy;
    const __amdgpu_buffer_rsrc_t r_uin = slice_rs(a.u_in + so, fbytes), r_in = slice_rs(a.in + so, fbytes);

    float Uc[RY + 3], In[RY];
#pragma unroll
    for (int r = 0; r < RY + 3; ++r) Uc[r] = ld_f(r_uin, xo, rowoff(r));
#pragma unroll
    for (int r = 0; r < RY; ++r) In[r] = ld_f(r_in, xo, rowoff(r + 2));

    // D of rows -1 .. RY-1 (index r + 1); reference naming: "x" differences run along rows, "y" along lanes
    float D1[RY + 1], D2[RY + 1];
#pragma unroll
    for (int r = -1; r < RY; ++r) {
        const int y = y0 + r;
        const float u = Uc[r + 2];
        const float ul = wave_prev(u), ur = wave_next(u);
        const float u_i1 = x_last ? ul : ur;
        const float u_i2 = x_first ? ur : ul;
        const float u_j1 = (y == dy - 1) ? Uc[r + 1] : Uc[r + 3];
        const float u_j2 = (y == 0) ? Uc[r + 3] : Uc[r + 1];
        const float nx1 = u_j1 - u, nx0 = u - u_j2;
        const float ny1 = u_i1 - u, ny0 = u - u_i2;
        const float dxm = rof_mm(nx0, nx1), dym = rof_mm(ny0, ny1);
        float d1 = rof_nrm(nx1, nx1 * nx1, dym, 0.0f);
        float d2 = rof_nrm(ny1, dxm, ny1 * ny1, 0.0f);
        if (HALF) { d1 = DualRt<__half>::rt(d1); d2 = DualRt<__half>::rt(d2); }
        D1[r + 1] = d1; D2[r + 1] = d2;
    }
    const __amdgpu_buffer_rsrc_t r_u = slice_rs(a.u_out + so, fbytes);
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const int y = y0 + r;
        // D1 of the reflected backward row (y-1, or y+1 at y == 0); D2 of the reflected backward lane
        const float d1b = (y == 0) ? D1[r + 2 <= RY ? r + 2 : RY] : D1[r];
        const float d2l = wave_prev(D2[r + 1]), d2r = wave_next(D2[r + 1]);
        const float d2b = x_first ? d2r : d2l;
        const float dv = (D1[r + 1] - d1b) + (D2[r + 1] - d2b);
        const float u = Uc[r + 2];
        const float tt = fmaf(a.lambda, dv, -(u - In[r]));
        const float uo = fmaf(a.tau, tt, u);
        if (emit_lane && y < dy) st_f(r_u, xo, y * pitch, uo);
    }
}

constexpr int ROF_RY = 8;  // rows per tile: rof_zmarch's

static int rof_slices_launch(const RofSliceArgs &a, int nslices, int half, hipStream_t st)
{
    int gx, gy, tiles;
    if (int rc = slice_tiles("ROF_TV", a.dx, a.dy, nslices, 60, ROF_RY, gx, gy, tiles)) return rc;
    if (half) rof_slices_kernel<true, ROF_RY><<<(unsigned)((tiles + 3) / 4), 256, 0, st>>>(a, gx, gy, tiles);
    else rof_slices_kernel<false, ROF_RY><<<(unsigned)((tiles + 3) / 4), 256, 0, st>>>(a, gx, gy, tiles);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

// the iterations of the next launch: pd_plan of tv_kernels.hip for a 2D image (3 per launch, 4 = 2 + 2)
inline int pd_next_k(int remaining) { return (remaining >= 3 && remaining != 4) ? 3 : remaining >= 2 ? 2 : 1; }

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
// Work arrays of tomo_pdtv_slices in the placed TV arena, each rounded up to 256 bytes and followed by the array skew:
// U ping-pong (float32), then P1, P2 of buffer set 0 and of buffer set 1 (float32 or binary16).
extern "C" size_t tomo_pdtv_slices_scratch_bytes(int dx, int dy, int nslices, int half)
{
    const size_t nvox = (size_t)dx * dy * nslices;
    return 2 * work_array_bytes(nvox) + 4 * (align_up(nvox * (half ? 2 : 4), 256) + WORK_SKEW);
}

// the one ping-pong partner of the output array
extern "C" size_t tomo_roftv_slices_scratch_bytes(int dx, int dy, int nslices)
{
    return work_array_bytes((size_t)dx * dy * nslices);
}

extern "C" int tomo_pdtv_slices(int device, const float *in_dev, float *out_dev, int dx, int dy, int nslices, float sigma,
                                float tau, float lt, float theta, int iters, int methodTV, int nonneg, int half, double tol,
                                int *iters_done, double *last_rel_change, void *stream)
{
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");
    TOMO_REQUIRE(dx > 0 && dy > 0 && nslices > 0 && iters >= 0, "bad PD_TV dimensions / iterations");
    TOMO_REQUIRE(tol >= 0.0 && std::isfinite(tol), "the tolerance must be a finite number >= 0");
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29), "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy);
    TOMO_REQUIRE(in_dev && out_dev, "NULL data pointer");
    const int v = g_variant_pdtv;
    TOMO_REQUIRE(v == 0 || v == 22, "slice-wise PD_TV runs the variants 0 and 22 only (selected: %d)", v);
    TOMO_ON_DEVICE(device);
    hipStream_t st = as_stream(stream);
    const size_t nvox = (size_t)dx * dy * nslices;
    if (iters_done) *iters_done = iters;
    if (last_rel_change) *last_rel_change = NAN;
    if (iters == 0) {
        if (out_dev != in_dev) TOMO_HIP(hipMemcpyAsync(out_dev, in_dev, nvox * sizeof(float), hipMemcpyDeviceToDevice, st));
        return TOMO_OK;
    }
    void *base = nullptr;
    int rc = tomo_arena_get(device, st, ARENA_TV, tomo_pdtv_slices_scratch_bytes(dx, dy, nslices, half), &base, true);
    if (rc != TOMO_OK) return rc;
    float *snap;
    rc = tol_snapshot(device, st, tol, iters, nvox, snap);
    if (rc != TOMO_OK) return rc;
    const size_t ub = work_array_bytes(nvox), pb = align_up(nvox * (half ? 2 : 4), 256) + WORK_SKEW;
    char *cur = (char *)base;
    float *U[2];
    void *P[2][2];
    U[0] = (float *)cur; cur += ub;
    U[1] = (float *)cur; cur += ub;
    for (int b = 0; b < 2; ++b)
        for (int c = 0; c < 2; ++c) { P[b][c] = cur; cur += pb; }
    tomo_prof_scope prof(PROF_PDTV, st, (iters + 2) / 3);
    // iteration 0 reads the caller's buffer (U[0] = data.copy() is not materialised) and no duals (they start at zero);
    // the last launch writes the caller's output (unless it aliases the input) and stores no duals
    int cset = 0;
    for (int it = 0; it < iters;) {
        const int k = pd_next_k(iters - it);
        const int ib = cset, ob = cset ^ 1;
        const bool last = (it + k == iters);
        PdSliceArgs a;
        a.in = in_dev;
        a.u_in = it == 0 ? in_dev : U[ib];
        a.u_out = (last && out_dev != in_dev) ? out_dev : U[ob];
        for (int c = 0; c < 2; ++c) { a.p_in[c] = P[ib][c]; a.p_out[c] = P[ob][c]; }
        a.dx = dx; a.dy = dy;
        a.sigma = sigma; a.tau = tau; a.lt = lt; a.theta = theta; a.inv1lt = 0.0f;
        a.p_in_zero = it == 0;
        a.p_out_skip = last;
        rc = pd_slices_dispatch(a, nslices, k, methodTV, nonneg, half, v, st);
        if (rc != TOMO_OK) return rc;
        cset = ob;
        it += k;
        // (every check point is a launch boundary: a multiple of 6 with at least 3 iterations left)
        if (!tol_due(snap, it, iters)) continue;
        TolCheck c;
        rc = tol_check(c, it, U[cset], in_dev, snap, nvox, tol, st);
        if (rc != TOMO_OK) return rc;
        if (last_rel_change) *last_rel_change = c.d;
        if (c.stop) {
            if (iters_done) *iters_done = it;
            TOMO_HIP(hipMemcpyAsync(out_dev, U[cset], nvox * sizeof(float), hipMemcpyDeviceToDevice, st));
            return TOMO_OK;
        }
    }
    if (out_dev == in_dev)
        TOMO_HIP(hipMemcpyAsync(out_dev, U[cset], nvox * sizeof(float), hipMemcpyDeviceToDevice, st));
    return TOMO_OK;
}

extern "C" int tomo_roftv_slices(int device, const float *in_dev, float *out_dev, int dx, int dy, int nslices, float lambda,
                                 float tau, int iters, int half, double tol, int *iters_done, double *last_rel_change,
                                 void *stream)
{
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");
    TOMO_REQUIRE(dx >= 2 && dy >= 2 && nslices >= 1 && iters >= 0, "ROF_TV needs every dimension >= 2 (reflecting boundary)");
    TOMO_REQUIRE(g_variant_roftv == 0, "slice-wise ROF_TV runs the variant 0 only (selected: %d)", g_variant_roftv);
    // (march_run checks these too, but only once the device is current: refuse them before it is touched, as every other entry does)
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29), "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy);
    TOMO_REQUIRE(in_dev && out_dev, "NULL data pointer");
    TOMO_ON_DEVICE(device);
    hipStream_t st = as_stream(stream);
    tomo_prof_scope prof(PROF_ROFTV, st, iters > 0 ? iters : 0);
    // the stack is march_run's "volume": U ping-pongs between the output array and one work array of the TV arena
    return march_run("ROF_TV", device, in_dev, out_dev, dx, dy, nslices, 3, iters, tol, iters_done, last_rel_change, stream,
                     [&](const float *u_in, float *u_out) {
                         const RofSliceArgs a{in_dev, u_in, u_out, dx, dy, lambda, tau};
                         return rof_slices_launch(a, nslices, half, st);
                     });
}
