// The launches that PDHG (primal-dual hybrid gradient, Chambolle-Pock, on the reconstruction problem itself:
//     min_x F(Ax) + lambda TV(x)  [+ x >= 0],   F = 1/2 |. - b|^2, |. - b|_1 or the Kullback-Leibler term)
// and SPDHG (its stochastic form over ordered subsets; Chambolle, Ehrhardt, Richtarik, Schoenlieb 2018: one block update
// touches one subset of angles or the TV block) add to the forward projector and the matched back projector for gfx950.
// There is no reference implementation in the tree: what is computed are the algorithms stated in docs/kernels/pdhg.md and
// docs/kernels/spdhg.md, formula-level parity, unpinned -- tests/_pdhg_oracle.py and tests/_spdhg_oracle.py restate them in
// numpy and the kernels reproduce their float32 form bit for bit (one rounding per operation in the stated order, no FMA
// contraction: -ffp-contract=off and no fmaf here; sqrtf and / are the compiler's correctly rounded ones).
//
// Both families run on ONE copy of three device skeletons; what a launch computes per element is a functor or a flag:
//   stream3_kernel<PdhgSino>        PDHG step 2:       y <- the prox of the conjugate of the data term at y + sigma r
//   stream3_kernel<StochSino>       SPDHG subset 2:    v = that prox on (y_j, r, b_j); d = v - y_j over r, y_j <- v
//   stream3_kernel<StochPrimal>     SPDHG subset 4:    z' = z + delta, zb = z' + w delta, x' = x - tau zb [clamped]
//   stream3_kernel<PdhgSinoDiag>    PDHG step 2 with a step per sample (the diagonal preconditioner): sigma_i from a 4th array
//   stream3_kernel<DiagSteps>       its set-up:        out = numer / max(in + add, 2^-10), the steps from the row / column sums
//   tv_dual_march<EMIT_E = false>   PDHG step 4:       q_d <- q_d + sigma F_d(x-bar), projected onto the ball or the box
//   tv_dual_march<EMIT_E = true>    SPDHG TV step 1:   the same p_d from x; e_d = p_d - q_d, q_d <- p_d
//   tv_primal_march<PdhgUpdate>     PDHG step 5:       x' = x - tau (g - div q) [clamped], x-bar = 2 x' - x
//   tv_primal_march<StochTvUpdate>  SPDHG TV 2, 3:     div = sum B_d(e_d); z' = z - div, zb = z' - w div, x' = x - tau zb
//   tv_primal_march<PdhgDiagUpdate> PDHG step 5 with a step per voxel: tau_j from one more plane stream
// and, with the second-order TGV term in PDHG's dual ("PD_TGV"), two marches of their own in pdhg_tgv.inl:
//   pdhg_tgv_dual_march             PDHG step 4:       P, Q <- the TGV dual update on x-bar, v-bar (88 B per voxel in 3D)
//   pdhg_tgv_primal_march<Update>   PDHG step 5:       PdhgUpdate / PdhgDiagUpdate on (x, g, div P), and v, v-bar (88 / 92 B)
// The streaming launches move 16 B (PdhgSino: r is not written), 20 B (PdhgSinoDiag too: 16 + the step) or, DiagSteps, 8 B
// per element.  The marches are plane marches on the
// skeleton of tgv_dual.inl / tgv_primal.inl (4 rows per lane, 2 x 2 waves, 63 columns per wave; the wave shifts, the plane
// I/O, the z-march grid and the array skew are the one copy in zmarch_common.h).  Each voxel's own values are read by that
// voxel only, and the neighbours a launch reads belong to fields it does not write, so nothing is ping-ponged.  Algorithmic
// traffic in 3D: the dual march 4 + 3 x 8 = 28 B (with e: 4 + 3 x 12 = 40 B), the primal march 3 x 4 + 8 + 8 = 28 B per voxel
// (PdhgDiagUpdate: + 4 = 32 B).
#include "zmarch_common.h"
#include "pdhg_data_term.h"
#include <initializer_list>

namespace {

// ------------------------------------------------------------------------------------------ the data term
// data_prox<MODE>, the prox of the conjugate of the data term at y + sigma r (step 2 of both algorithms): pdhg_data_term.h
//
// The per-element functors of stream3_kernel: op(a, b, c) updates a, and b where WRITES_B says so.  STEP_ARRAY: the functor
// carries a fourth array, `step`, read beside the three, and is called as op(a, b, c, step[i]).
template <int MODE>
struct PdhgSino {   // y <- v
    static constexpr bool WRITES_B = false, STEP_ARRAY = false;
    float sigma, one_sigma, c4;
    __device__ __forceinline__ void operator()(float &y, float &r, float b) const { y = data_prox<MODE>(y, r, b, sigma, one_sigma, c4); }
};

template <int MODE>
struct PdhgSinoDiag {   // y <- v with sigma_i = step[i]
    static constexpr bool WRITES_B = false, STEP_ARRAY = true;
    const float *step;
    __device__ __forceinline__ void operator()(float &y, float &r, float b, float sigma) const
    {
        y = data_prox<MODE>(y, r, b, sigma, 1.0f + sigma, 4.0f * sigma);
    }
};

struct DiagSteps {   // a <- numer / max(c + add, eps): neither a nor b is read, so the launch streams c in and a out
    static constexpr bool WRITES_B = false, STEP_ARRAY = false;
    float numer, add, eps;
    __device__ __forceinline__ void operator()(float &out, float &, float in) const
    {
        const float v = in + add;
        out = numer / (v < eps ? eps : v);
    }
};

template <int MODE>
struct StochSino {   // y <- v and r <- d = v - y
    static constexpr bool WRITES_B = true, STEP_ARRAY = false;
    float sigma, one_sigma, c4;
    __device__ __forceinline__ void operator()(float &y, float &r, float b) const
    {
        const float v = data_prox<MODE>(y, r, b, sigma, one_sigma, c4);
        r = v - y;
        y = v;
    }
};

struct StochPrimal {   // SPDHG subset step 4
    static constexpr bool WRITES_B = true, STEP_ARRAY = false;
    float tau, w;
    int nonneg;
    __device__ __forceinline__ void operator()(float &x, float &z, float delta) const
    {
        const float zn = z + delta;
        const float zb = zn + w * delta;
        float xn = x - tau * zb;
        if (nonneg) xn = xn < 0.0f ? 0.0f : xn;
        x = xn;
        z = zn;
    }
};

// ------------------------------------------------------------------------------------------ the streaming skeleton
constexpr int STREAM_BLOCK = 256;
constexpr int STREAM_MAX_GRID = 256 * 8;   // 256 CUs x 8 blocks, grid-stride beyond

// element i in scalar form
template <class Op>
__device__ __forceinline__ void stream3_one(const Op &op, float *a, float *b, const float *c, size_t i)
{
    float sa = a[i], sb = b[i];
    if constexpr (Op::STEP_ARRAY) op(sa, sb, c[i], op.step[i]);
    else op(sa, sb, c[i]);
    a[i] = sa;
    if (Op::WRITES_B) b[i] = sb;
}

// Three arrays of n floats: a is read and written, b is read (and written: Op::WRITES_B), c is read.
// VEC: 16-byte accesses over the first n / 4 quads and a scalar tail by block 0 (all three arrays, and the step array of
// an Op::STEP_ARRAY functor, 16-byte aligned)
template <class Op, bool VEC>
__global__ __launch_bounds__(STREAM_BLOCK) void stream3_kernel(float *a, float *b, const float *c, size_t n, Op op)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const size_t n4 = n >> 2;
        for (size_t i = first; i < n4; i += stride) {
            float4 va = reinterpret_cast<const float4 *>(a)[i];
            float4 vb = reinterpret_cast<const float4 *>(b)[i];
            const float4 vc = reinterpret_cast<const float4 *>(c)[i];
            if constexpr (Op::STEP_ARRAY) {
                const float4 vs = reinterpret_cast<const float4 *>(op.step)[i];
                op(va.x, vb.x, vc.x, vs.x);
                op(va.y, vb.y, vc.y, vs.y);
                op(va.z, vb.z, vc.z, vs.z);
                op(va.w, vb.w, vc.w, vs.w);
            } else {
                op(va.x, vb.x, vc.x);
                op(va.y, vb.y, vc.y);
                op(va.z, vb.z, vc.z);
                op(va.w, vb.w, vc.w);
            }
            reinterpret_cast<float4 *>(a)[i] = va;
            if (Op::WRITES_B) reinterpret_cast<float4 *>(b)[i] = vb;
        }
        const size_t i = (n4 << 2) + threadIdx.x;
        if (blockIdx.x == 0 && i < n) stream3_one(op, a, b, c, i);
    } else {
        for (size_t i = first; i < n; i += stride) stream3_one(op, a, b, c, i);
    }
}

// the only launch site of the streaming skeleton
template <class Op>
static void stream3_launch(float *a, float *b, const float *c, size_t n, Op op, hipStream_t st)
{
    uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c);
    if constexpr (Op::STEP_ARRAY) bits |= reinterpret_cast<uintptr_t>(op.step);
    const bool vec = (bits & 15u) == 0;
    const size_t items = vec ? (n >> 2) : n;
    size_t grid = (items + STREAM_BLOCK - 1) / STREAM_BLOCK;
    if (grid < 1) grid = 1;
    if (grid > (size_t)STREAM_MAX_GRID) grid = STREAM_MAX_GRID;
    if (vec)
        stream3_kernel<Op, true><<<(unsigned)grid, STREAM_BLOCK, 0, st>>>(a, b, c, n, op);
    else
        stream3_kernel<Op, false><<<(unsigned)grid, STREAM_BLOCK, 0, st>>>(a, b, c, n, op);
}

// the sinogram dual of either family over the three data terms
template <template <int> class Sino>
static void sino_launch(int fidelity, float *y, float *r, const float *b, size_t n, float sigma, hipStream_t st)
{
    const float one_sigma = 1.0f + sigma, c4 = 4.0f * sigma;
    if (fidelity == TOMO_PDHG_LS) stream3_launch(y, r, b, n, Sino<TOMO_PDHG_LS>{sigma, one_sigma, c4}, st);
    else if (fidelity == TOMO_PDHG_L1) stream3_launch(y, r, b, n, Sino<TOMO_PDHG_L1>{sigma, one_sigma, c4}, st);
    else stream3_launch(y, r, b, n, Sino<TOMO_PDHG_KL>{sigma, one_sigma, c4}, st);
}

// the same with a step per sample
static void sino_diag_launch(int fidelity, float *y, float *r, const float *b, const float *sigma, size_t n, hipStream_t st)
{
    if (fidelity == TOMO_PDHG_LS) stream3_launch(y, r, b, n, PdhgSinoDiag<TOMO_PDHG_LS>{sigma}, st);
    else if (fidelity == TOMO_PDHG_L1) stream3_launch(y, r, b, n, PdhgSinoDiag<TOMO_PDHG_L1>{sigma}, st);
    else stream3_launch(y, r, b, n, PdhgSinoDiag<TOMO_PDHG_KL>{sigma}, st);
}

// ------------------------------------------------------------------------------------------ the forward-difference march
struct TvDualArgs {
    const float *src;  // the field whose gradient is taken: PDHG's x-bar, SPDHG's x
    float *q[3];       // the TV dual
    float *e[3];       // its change p - q of this update (EMIT_E only)
    int dx, dy, dz;
    float sigma, lambda;
};

// p_d = q_d + sigma F_d(src), projected onto the ball (isotropic) or the box (anisotropic); q_d <- p_d and, with EMIT_E,
// e_d <- p_d - q_d.  A lane owns RY rows of one x column and walks z.  The +x neighbour is the next lane (lane 63 of a wave
// is a halo lane: 63 columns per wave), the +y neighbour the next register (one halo row below the tile), the +z neighbour
// the plane loaded one step ahead, which becomes the current plane of the next step: src is read once per launch (plus
// halos), q read and written once, e written once.
template <int ND, bool ANISO, bool EMIT_E, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void tv_dual_march(TvDualArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
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
    for (int q = 0; q <= RY; ++q) cur[q] = io.ld(a.src + sz * zc0, xo, rowoff(q));

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_next = t < dz - 1;
        if (ND == 3) {
            const size_t pn = sz * min(t + 1, dz - 1);
#pragma unroll
            for (int q = 0; q <= RY; ++q) nxt[q] = io.ld(a.src + pn, xo, rowoff(q));
        }
        float Q[ND][RY], E[ND][RY];
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int r = 0; r < RY; ++r) Q[d][r] = io.ld(a.q[d] + sz * t, xo, rowoff(r));

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_next = y0 + r < dy - 1;
            // F_d(src): a[i + e_d] - a[i], exactly 0 on the last index of the axis
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
                    if (EMIT_E) io.st(a.e[d] + sz * t, xo, rowoff(r), E[d][r]);
                }
            }
        }
        if (ND == 3) {
#pragma unroll
            for (int q = 0; q <= RY; ++q) cur[q] = nxt[q];
        }
    }
}

// ------------------------------------------------------------------------------------------ the backward-difference march
struct TvPrimalArgs {
    float *x;          // the primal variable
    const float *s;    // the second array the update reads: PDHG's g = A^T y, SPDHG's z = sum K_j^T y_j
    float *s_out;      // the second array it writes: PDHG's x-bar, SPDHG's z (Update::IN_PLACE: the same array)
    const float *f[3]; // the fields whose divergence is taken: PDHG's q, SPDHG's e (TV = false: none, div = 0)
    int dx, dy, dz;
};

// The per-voxel functors of tv_primal_march: (X, S, div) -> the new x and the second output; IN_PLACE: the second output
// replaces the second input.  STEP_ARRAY: the functor carries one more field, `step`, read at the lane's own voxels like x,
// and is called as update(X, S, div, step[i]).
struct XS {   // what an update returns: the new x and the second output
    float x, s;
};

struct PdhgUpdate {   // x' = x - tau (g - div) [clamped], x-bar = 2 x' - x
    static constexpr bool IN_PLACE = false, STEP_ARRAY = false;
    float tau;
    int nonneg;
    __device__ __forceinline__ XS operator()(float X, float G, float div) const
    {
        float xn = X - tau * (G - div);
        if (nonneg) xn = xn < 0.0f ? 0.0f : xn;
        return {xn, (xn + xn) - X};
    }
};

struct PdhgDiagUpdate {   // the same with tau_j = step[j]
    static constexpr bool IN_PLACE = false, STEP_ARRAY = true;
    const float *step;
    int nonneg;
    __device__ __forceinline__ XS operator()(float X, float G, float div, float tau) const
    {
        return PdhgUpdate{tau, nonneg}(X, G, div);
    }
};

struct StochTvUpdate {   // z' = z - div, zb = z' - w div, x' = x - tau zb [clamped]
    static constexpr bool IN_PLACE = true, STEP_ARRAY = false;
    float tau, w;
    int nonneg;
    __device__ __forceinline__ XS operator()(float X, float Z, float div) const
    {
        const float zn = Z - div;
        const float zb = zn - w * div;
        float xn = X - tau * zb;
        if (nonneg) xn = xn < 0.0f ? 0.0f : xn;
        return {xn, zn};
    }
};

// The mirror image of tv_dual_march: the -x neighbour is the previous lane (lane 0 of a wave is the halo lane), the -y
// neighbour the previous register (one halo row above the tile, f2 only), the -z neighbour the carried registers of the
// plane before (f3; a z-chunk loads them once for the plane below its first).  f is read and not written; x and s (and the
// step field of an Update::STEP_ARRAY functor) are read and x and s_out written at the lane's own voxels only.  div = (B_1 f_1 + B_2 f_2) + B_3 f_3.
template <int ND, bool TV, class Update, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void tv_primal_march(TvPrimalArgs a, Update update, int gx, int gy, int tiles_per_xcd,
                                                               int zchunk)
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
    const float *s = Update::IN_PLACE ? a.s_out : a.s;   // one pointer where the two are one array
    // slot q = row y0 - 1 + q (q = 0: the halo row), clamped into the plane
    auto rowoff = [&](int q) __attribute__((always_inline)) { return min(max(wy0 - 1 + q, 0), dy - 1) * pitch; };

    // the plane below: f3
    float Zp[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) Zp[r] = 0.0f;
    if (TV && ND == 3 && zc0 > 0) {
#pragma unroll
        for (int r = 0; r < RY; ++r) Zp[r] = io.ld(a.f[ND - 1] + sz * (zc0 - 1), xo, rowoff(r + 1));
    }

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_prev = t > 0;
        const size_t pt = sz * t;
        float F1[RY], F2[RY + 1], F3[RY], X[RY], S[RY], T[RY];
        if (TV) {
#pragma unroll
            for (int q = 0; q <= RY; ++q) F2[q] = io.ld(a.f[1] + pt, xo, rowoff(q));
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (TV) {
                F1[r] = io.ld(a.f[0] + pt, xo, rowoff(r + 1));
                if (ND == 3) F3[r] = io.ld(a.f[ND - 1] + pt, xo, rowoff(r + 1));
            }
            X[r] = io.ld(a.x + pt, xo, rowoff(r + 1));
            S[r] = io.ld(s + pt, xo, rowoff(r + 1));
            if constexpr (Update::STEP_ARRAY) T[r] = io.ld(update.step + pt, xo, rowoff(r + 1));
        }

        float Xn[RY], Sn[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            float div = 0.0f;
            if (TV) {
                const bool y_prev = y0 + r > 0;
                // B_d(a)[i] = a[i] - a[i - e_d], a[i] itself on the first index of the axis
                const float l = wave_prev(F1[r]);
                div = (x_prev ? F1[r] - l : F1[r]) + (y_prev ? F2[r + 1] - F2[r] : F2[r + 1]);
                if (ND == 3) {
                    div = div + (z_prev ? F3[r] - Zp[r] : F3[r]);
                    Zp[r] = F3[r];
                }
            }
            XS o;
            if constexpr (Update::STEP_ARRAY) o = update(X[r], S[r], div, T[r]);
            else o = update(X[r], S[r], div);
            Xn[r] = o.x;
            Sn[r] = o.s;
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) {
                io.st(a.x + pt, xo, rowoff(r + 1), Xn[r]);
                io.st(a.s_out + pt, xo, rowoff(r + 1), Sn[r]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ the host side of the marches
// The only launch sites of the two marches: TGV's tile, 4 rows per lane, 2 x 2 waves, 63 columns per wave.  `op` names the
// operator in messages.
template <int ND, bool ANISO, bool EMIT_E>
static int tv_dual_launch(const char *op, const TvDualArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, op, a.dx, a.dy, a.dz, 63, 2, 2, 4, ND == 3)) return rc;
    tv_dual_march<ND, ANISO, EMIT_E, 4, 2, 2><<<(unsigned)g.blocks, 64 * 2 * 2, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

template <int ND, bool TV, class Update>
static int tv_primal_launch(const char *op, const TvPrimalArgs &a, Update update, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, op, a.dx, a.dy, a.dz, 63, 2, 2, 4, ND == 3)) return rc;
    tv_primal_march<ND, TV, Update, 4, 2, 2><<<(unsigned)g.blocks, 64 * 2 * 2, 0, st>>>(a, update, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

template <bool EMIT_E>
static int tv_dual_run(const char *op, const TvDualArgs &a, int nd, int methodTV, hipStream_t st)
{
    return nd == 3 ? (methodTV ? tv_dual_launch<3, true, EMIT_E>(op, a, st) : tv_dual_launch<3, false, EMIT_E>(op, a, st))
                   : (methodTV ? tv_dual_launch<2, true, EMIT_E>(op, a, st) : tv_dual_launch<2, false, EMIT_E>(op, a, st));
}

// the checks the marches share; `dz` becomes 1 for nd = 2
static int require_volume(const char *op, int device, int dx, int dy, int &dz, int nd)
{
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");
    TOMO_REQUIRE(nd == 2 || nd == 3, "2D or 3D arrays must be provided only");
    if (nd == 2) dz = 1;
    TOMO_REQUIRE(dx >= 1 && dy >= 1 && dz >= 1, "%s needs every dimension >= 1", op);
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29),
                 "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy);
    return TOMO_OK;
}

// no two of the pointers are equal (null pointers excepted)
static bool distinct(std::initializer_list<const float *> ptrs)
{
    for (auto i = ptrs.begin(); i != ptrs.end(); ++i)
        for (auto k = i + 1; k != ptrs.end(); ++k)
            if (*i && *i == *k) return false;
    return true;
}

#include "pdhg_tgv.inl"

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI: PDHG
extern "C" size_t tomo_pdhg_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    return (size_t)(2 + nd) * work_array_bytes((size_t)dx * dy * dz);   // x-bar, g, q_1..q_nd
}

extern "C" int tomo_pdhg_sino_dual(float *y_dev, const float *r_dev, const float *b_dev, size_t count, int fidelity,
                                   float sigma, void *stream)
{
    TOMO_REQUIRE(known_fidelity(fidelity), "PDHG: the data term must be TOMO_PDHG_LS, TOMO_PDHG_L1 or TOMO_PDHG_KL");
    TOMO_REQUIRE(positive_finite(sigma), "PDHG: the step size sigma must be positive");
    TOMO_REQUIRE(y_dev && r_dev && b_dev, "NULL data pointer");
    TOMO_REQUIRE(y_dev != r_dev && y_dev != b_dev, "PDHG: the dual array must not alias an array the launch reads");
    if (count == 0) return TOMO_OK;
    sino_launch<PdhgSino>(fidelity, y_dev, const_cast<float *>(r_dev) /* PdhgSino does not write it */, b_dev, count, sigma,
                          as_stream(stream));
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

extern "C" size_t tomo_pdhg_diag_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    return tomo_pdhg_scratch_bytes(dx, dy, dz, nd) + work_array_bytes((size_t)dx * dy * dz);   // ... and tau, behind them
}

extern "C" int tomo_pdhg_diag_steps(float *out_dev, const float *in_dev, size_t count, float numer, float add, void *stream)
{
    TOMO_REQUIRE(positive_finite(numer), "PDHG: the numerator of the steps must be positive");
    TOMO_REQUIRE(add >= 0.0f && std::isfinite(add), "PDHG: the constant added to the sums must be finite and not negative");
    TOMO_REQUIRE(out_dev && in_dev, "NULL data pointer");
    if (count == 0) return TOMO_OK;
    // the skeleton's second array is neither read nor written by DiagSteps: it only takes part in the alignment test
    stream3_launch(out_dev, out_dev, in_dev, count, DiagSteps{numer, add, 0x1p-10f}, as_stream(stream));
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

extern "C" int tomo_pdhg_sino_dual_diag(float *y_dev, const float *r_dev, const float *b_dev, const float *sigma_dev, size_t count,
                                        int fidelity, void *stream)
{
    TOMO_REQUIRE(known_fidelity(fidelity), "PDHG: the data term must be TOMO_PDHG_LS, TOMO_PDHG_L1 or TOMO_PDHG_KL");
    TOMO_REQUIRE(y_dev && r_dev && b_dev && sigma_dev, "NULL data pointer");
    TOMO_REQUIRE(y_dev != r_dev && y_dev != b_dev && y_dev != sigma_dev, "PDHG: the dual array must not alias an array the launch reads");
    if (count == 0) return TOMO_OK;
    sino_diag_launch(fidelity, y_dev, const_cast<float *>(r_dev) /* PdhgSinoDiag does not write it */, b_dev, sigma_dev, count,
                     as_stream(stream));
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

extern "C" int tomo_pdhg_tv_dual(int device, const float *xbar_dev, float *q1_dev, float *q2_dev, float *q3_dev, int dx,
                                 int dy, int dz, int nd, float sigma, float lambda, int methodTV, void *stream)
{
    if (int rc = require_volume("PDHG", device, dx, dy, dz, nd)) return rc;
    TOMO_REQUIRE(methodTV == 0 || methodTV == 1, "PDHG: methodTV must be 0 (isotropic) or 1 (anisotropic)");
    TOMO_REQUIRE(positive_finite(sigma), "PDHG: the step size sigma must be positive");
    TOMO_REQUIRE(positive_finite(lambda), "PDHG: lambda must be positive");
    TOMO_REQUIRE(xbar_dev && q1_dev && q2_dev && (nd == 2 || q3_dev), "NULL data pointer");
    TOMO_REQUIRE(distinct({xbar_dev, q1_dev, q2_dev, q3_dev}), "PDHG: the dual fields must not alias each other or x-bar");
    TOMO_ON_DEVICE(device);
    const TvDualArgs a{xbar_dev, {q1_dev, q2_dev, nd == 3 ? q3_dev : nullptr}, {}, dx, dy, dz, sigma, lambda};
    return tv_dual_run<false>("PDHG", a, nd, methodTV, as_stream(stream));
}

// what tomo_pdhg_primal and tomo_pdhg_primal_diag share: the checks and the choice of the instantiation; `tau_dev`, where
// given, is one more array the launch reads
template <class Update>
static int pdhg_primal_run(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *tau_dev, const float *q1_dev,
                           const float *q2_dev, const float *q3_dev, int dx, int dy, int dz, int nd, Update update, void *stream)
{
    const bool tv = q1_dev != nullptr;
    TOMO_REQUIRE(tv ? (q2_dev && (nd == 2 || q3_dev)) : (!q2_dev && !q3_dev),
                 "PDHG: give every dual field of the TV block (q3 for nd = 3 only) or none");
    TOMO_REQUIRE(distinct({x_dev, xbar_dev, g_dev, tau_dev}), "PDHG: x, x-bar, g and the step array must not alias");
    for (const float *q : {q1_dev, q2_dev, q3_dev})
        TOMO_REQUIRE(!q || (q != x_dev && q != xbar_dev), "PDHG: a dual field must not alias an array the launch writes");
    TOMO_ON_DEVICE(device);
    const TvPrimalArgs a{x_dev, g_dev, xbar_dev, {q1_dev, q2_dev, nd == 3 ? q3_dev : nullptr}, dx, dy, dz};
    hipStream_t st = as_stream(stream);
    return nd == 3 ? (tv ? tv_primal_launch<3, true>("PDHG", a, update, st) : tv_primal_launch<3, false>("PDHG", a, update, st))
                   : (tv ? tv_primal_launch<2, true>("PDHG", a, update, st) : tv_primal_launch<2, false>("PDHG", a, update, st));
}

extern "C" int tomo_pdhg_primal(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *q1_dev,
                                const float *q2_dev, const float *q3_dev, int dx, int dy, int dz, int nd, float tau,
                                int nonneg, void *stream)
{
    if (int rc = require_volume("PDHG", device, dx, dy, dz, nd)) return rc;
    TOMO_REQUIRE(positive_finite(tau), "PDHG: the step size tau must be positive");
    TOMO_REQUIRE(x_dev && xbar_dev && g_dev, "NULL data pointer");
    return pdhg_primal_run(device, x_dev, xbar_dev, g_dev, nullptr, q1_dev, q2_dev, q3_dev, dx, dy, dz, nd,
                           PdhgUpdate{tau, nonneg ? 1 : 0}, stream);
}

extern "C" int tomo_pdhg_primal_diag(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *tau_dev,
                                     const float *q1_dev, const float *q2_dev, const float *q3_dev, int dx, int dy, int dz, int nd,
                                     int nonneg, void *stream)
{
    if (int rc = require_volume("PDHG", device, dx, dy, dz, nd)) return rc;
    TOMO_REQUIRE(x_dev && xbar_dev && g_dev && tau_dev, "NULL data pointer");
    return pdhg_primal_run(device, x_dev, xbar_dev, g_dev, tau_dev, q1_dev, q2_dev, q3_dev, dx, dy, dz, nd,
                           PdhgDiagUpdate{tau_dev, nonneg ? 1 : 0}, stream);
}

// ------------------------------------------------------------------------------------------ C-ABI: PDHG with TGV in the dual
extern "C" size_t tomo_pdhg_tgv_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    const size_t narr = nd == 2 ? 11 : 17;   // x-bar, g, P, v, v-bar (nd each), Q (3 or 6)
    return narr * work_array_bytes((size_t)dx * dy * dz);
}

extern "C" size_t tomo_pdhg_tgv_diag_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    return tomo_pdhg_tgv_scratch_bytes(dx, dy, dz, nd) + work_array_bytes((size_t)dx * dy * dz);   // ... and tau, behind them
}

// the fields of the TGV block as the entry points take them: host arrays of nd (v, v-bar, P) and 3 or 6 (Q) device pointers
static bool all_given(const float *const *fields, int count)
{
    if (!fields) return false;
    for (int k = 0; k < count; ++k)
        if (!fields[k]) return false;
    return true;
}

extern "C" int tomo_pdhg_tgv_dual(int device, const float *xbar_dev, const float *const *vbar_dev, float *const *p_dev,
                                  float *const *q_dev, int dx, int dy, int dz, int nd, float sigma_p, float sigma_q, float r1,
                                  float r0, void *stream)
{
    if (int rc = require_volume("PDHG", device, dx, dy, dz, nd)) return rc;
    const int nq = nd == 3 ? 6 : 3;
    TOMO_REQUIRE(positive_finite(sigma_p) && positive_finite(sigma_q), "PDHG: the step sizes sigma_P and sigma_Q must be positive");
    TOMO_REQUIRE(positive_finite(r1) && positive_finite(r0), "PDHG: the radii lambda alpha1 and lambda alpha0 must be positive");
    TOMO_REQUIRE(xbar_dev && all_given(vbar_dev, nd) && all_given(p_dev, nd) && all_given(q_dev, nq), "NULL data pointer");
    TgvDualArgs a{};
    a.xb = xbar_dev;
    for (int c = 0; c < nd; ++c) { a.vb[c] = vbar_dev[c]; a.p[c] = p_dev[c]; }
    for (int k = 0; k < nq; ++k) a.q[k] = q_dev[k];
    TOMO_REQUIRE(distinct({a.xb, a.vb[0], a.vb[1], a.vb[2], a.p[0], a.p[1], a.p[2], a.q[0], a.q[1], a.q[2], a.q[3], a.q[4], a.q[5]}),
                 "PDHG: the dual fields P and Q must not alias each other, x-bar or v-bar");
    TOMO_ON_DEVICE(device);
    a.dx = dx; a.dy = dy; a.dz = dz;
    a.sigma_p = sigma_p; a.sigma_q = sigma_q; a.r1 = r1; a.r0 = r0;
    hipStream_t st = as_stream(stream);
    return nd == 3 ? pdhg_tgv_dual_launch<3>(a, st) : pdhg_tgv_dual_launch<2>(a, st);
}

// what tomo_pdhg_tgv_primal and tomo_pdhg_tgv_primal_diag share: the checks and the choice of the instantiation; `tau_dev`,
// where given, is one more array the launch reads
template <class Update>
static int pdhg_tgv_primal_run(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *tau_dev,
                               float *const *v_dev, float *const *vbar_dev, const float *const *p_dev, const float *const *q_dev,
                               int dx, int dy, int dz, int nd, float tau_v, Update update, void *stream)
{
    const int nq = nd == 3 ? 6 : 3;
    TOMO_REQUIRE(positive_finite(tau_v), "PDHG: the step size tau_v must be positive");
    TOMO_REQUIRE(all_given(v_dev, nd) && all_given(vbar_dev, nd) && all_given(p_dev, nd) && all_given(q_dev, nq), "NULL data pointer");
    TgvPrimalArgs a{};
    a.x = x_dev; a.xb = xbar_dev; a.g = g_dev;
    for (int c = 0; c < nd; ++c) { a.v[c] = v_dev[c]; a.vb[c] = vbar_dev[c]; a.p[c] = p_dev[c]; }
    for (int k = 0; k < nq; ++k) a.q[k] = q_dev[k];
    TOMO_REQUIRE(distinct({a.x, a.xb, a.g, tau_dev, a.v[0], a.v[1], a.v[2], a.vb[0], a.vb[1], a.vb[2], a.p[0], a.p[1], a.p[2],
                           a.q[0], a.q[1], a.q[2], a.q[3], a.q[4], a.q[5]}),
                 "PDHG: x, x-bar, g, the step array, v, v-bar, P and Q must not alias");
    TOMO_ON_DEVICE(device);
    a.dx = dx; a.dy = dy; a.dz = dz;
    a.tau_v = tau_v;
    hipStream_t st = as_stream(stream);
    return nd == 3 ? pdhg_tgv_primal_launch<3>(a, update, st) : pdhg_tgv_primal_launch<2>(a, update, st);
}

extern "C" int tomo_pdhg_tgv_primal(int device, float *x_dev, float *xbar_dev, const float *g_dev, float *const *v_dev,
                                    float *const *vbar_dev, const float *const *p_dev, const float *const *q_dev, int dx, int dy,
                                    int dz, int nd, float tau_x, float tau_v, int nonneg, void *stream)
{
    if (int rc = require_volume("PDHG", device, dx, dy, dz, nd)) return rc;
    TOMO_REQUIRE(positive_finite(tau_x), "PDHG: the step size tau_x must be positive");
    TOMO_REQUIRE(x_dev && xbar_dev && g_dev, "NULL data pointer");
    return pdhg_tgv_primal_run(device, x_dev, xbar_dev, g_dev, nullptr, v_dev, vbar_dev, p_dev, q_dev, dx, dy, dz, nd, tau_v,
                               PdhgUpdate{tau_x, nonneg ? 1 : 0}, stream);
}

extern "C" int tomo_pdhg_tgv_primal_diag(int device, float *x_dev, float *xbar_dev, const float *g_dev, const float *tau_dev,
                                         float *const *v_dev, float *const *vbar_dev, const float *const *p_dev,
                                         const float *const *q_dev, int dx, int dy, int dz, int nd, float tau_v, int nonneg,
                                         void *stream)
{
    if (int rc = require_volume("PDHG", device, dx, dy, dz, nd)) return rc;
    TOMO_REQUIRE(x_dev && xbar_dev && g_dev && tau_dev, "NULL data pointer");
    return pdhg_tgv_primal_run(device, x_dev, xbar_dev, g_dev, tau_dev, v_dev, vbar_dev, p_dev, q_dev, dx, dy, dz, nd, tau_v,
                               PdhgDiagUpdate{tau_dev, nonneg ? 1 : 0}, stream);
}

// ------------------------------------------------------------------------------------------ C-ABI: SPDHG
extern "C" size_t tomo_spdhg_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    return (size_t)(2 + 2 * nd) * work_array_bytes((size_t)dx * dy * dz);   // z, delta, q_1..q_nd, e_1..e_nd
}

extern "C" int tomo_spdhg_sino_dual(float *y_dev, float *r_dev, const float *b_dev, size_t count, int fidelity, float sigma,
                                    void *stream)
{
    TOMO_REQUIRE(known_fidelity(fidelity), "SPDHG: the data term must be TOMO_PDHG_LS, TOMO_PDHG_L1 or TOMO_PDHG_KL");
    TOMO_REQUIRE(positive_finite(sigma), "SPDHG: the step size sigma must be positive");
    TOMO_REQUIRE(y_dev && r_dev && b_dev, "NULL data pointer");
    TOMO_REQUIRE(distinct({y_dev, r_dev, b_dev}), "SPDHG: the dual array, the projection and the data must not alias");
    if (count == 0) return TOMO_OK;
    sino_launch<StochSino>(fidelity, y_dev, r_dev, b_dev, count, sigma, as_stream(stream));
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
    stream3_launch(x_dev, z_dev, delta_dev, count, StochPrimal{tau, w, nonneg ? 1 : 0}, as_stream(stream));
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

extern "C" int tomo_spdhg_tv_dual(int device, const float *x_dev, float *q1_dev, float *q2_dev, float *q3_dev, float *e1_dev,
                                  float *e2_dev, float *e3_dev, int dx, int dy, int dz, int nd, float sigma, float lambda,
                                  int methodTV, void *stream)
{
    if (int rc = require_volume("SPDHG", device, dx, dy, dz, nd)) return rc;
    TOMO_REQUIRE(methodTV == 0 || methodTV == 1, "SPDHG: methodTV must be 0 (isotropic) or 1 (anisotropic)");
    TOMO_REQUIRE(positive_finite(sigma), "SPDHG: the step size sigma must be positive");
    TOMO_REQUIRE(positive_finite(lambda), "SPDHG: lambda must be positive");
    TOMO_REQUIRE(x_dev && q1_dev && q2_dev && e1_dev && e2_dev && (nd == 2 || (q3_dev && e3_dev)), "NULL data pointer");
    if (nd == 2) q3_dev = e3_dev = nullptr;
    TOMO_REQUIRE(distinct({x_dev, q1_dev, q2_dev, q3_dev, e1_dev, e2_dev, e3_dev}),
                 "SPDHG: the dual fields and their changes must not alias each other or x");
    TOMO_ON_DEVICE(device);
    const TvDualArgs a{x_dev, {q1_dev, q2_dev, q3_dev}, {e1_dev, e2_dev, e3_dev}, dx, dy, dz, sigma, lambda};
    return tv_dual_run<true>("SPDHG", a, nd, methodTV, as_stream(stream));
}

extern "C" int tomo_spdhg_tv_primal(int device, float *x_dev, float *z_dev, const float *e1_dev, const float *e2_dev,
                                    const float *e3_dev, int dx, int dy, int dz, int nd, float tau, float w, int nonneg,
                                    void *stream)
{
    if (int rc = require_volume("SPDHG", device, dx, dy, dz, nd)) return rc;
    TOMO_REQUIRE(positive_finite(tau), "SPDHG: the step size tau must be positive");
    TOMO_REQUIRE(positive_finite(w), "SPDHG: the extrapolation weight w (1 / the block's probability) must be positive");
    TOMO_REQUIRE(x_dev && z_dev && e1_dev && e2_dev && (nd == 2 || e3_dev), "NULL data pointer");
    if (nd == 2) e3_dev = nullptr;
    TOMO_REQUIRE(distinct({x_dev, z_dev, e1_dev, e2_dev, e3_dev}), "SPDHG: x, z and the changes of the dual fields must not alias");
    TOMO_ON_DEVICE(device);
    const TvPrimalArgs a{x_dev, z_dev, z_dev, {e1_dev, e2_dev, e3_dev}, dx, dy, dz};
    const StochTvUpdate update{tau, w, nonneg ? 1 : 0};
    hipStream_t st = as_stream(stream);
    return nd == 3 ? tv_primal_launch<3, true>("SPDHG", a, update, st) : tv_primal_launch<2, true>("SPDHG", a, update, st);
}
