// The two launches PDHG runs per iteration with the second-order TGV term in its dual ("PD_TGV", docs/kernels/pdhg.md):
//   pdhg_tgv_dual_march    step 4: P and Q ascend along the forward differences of x-bar and v-bar and are projected onto
//                          their balls, in place -- the work of tgv_dual.inl with a step of its own for P and for Q
//   pdhg_tgv_primal_march  step 5: x' = x - tau_x (g - div P) [clamped], x-bar = 2 x' - x -- PdhgUpdate / PdhgDiagUpdate, the
//                          functors of tv_primal_march -- joined to step 4 of tgv_primal.inl for v and v-bar
// Included inside the anonymous namespace of pdhg_kernels.hip (PlaneIO, wave_next, wave_prev and zmarch_grid of
// zmarch_common.h; PdhgUpdate, PdhgDiagUpdate, XS).  Both are plane marches on TGV's tile: a lane owns RY rows of one x
// column and walks z, 63 columns per wave, the x neighbour a DPP wave shift, the y neighbour a register, the z neighbour the
// plane loaded one step ahead (dual) or carried from the step before (primal).  Each voxel's own values are read by that
// voxel only, and the neighbours a launch reads belong to fields it does not write, so nothing is ping-ponged and nothing
// goes through LDS.  Algorithmic traffic in 3D: the dual 4 x 4 + 9 x 8 = 88 B, the primal 9 x 4 + 4 + 4 x 12 = 88 B per voxel
// (a step per voxel: + 4 = 92 B); in 2D 52 B and 60 B (64 B).

// Q components; 2D uses the first three
enum { GQ11 = 0, GQ22 = 1, GQ12 = 2, GQ33 = 3, GQ13 = 4, GQ23 = 5 };

struct TgvDualArgs {
    const float *xb;       // x-bar
    const float *vb[3];    // v-bar
    float *p[3], *q[6];    // the two duals of the TGV block
    int dx, dy, dz;
    float sigma_p, sigma_q, r1, r0;
};

template <int ND, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void pdhg_tgv_dual_march(TgvDualArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
{
    constexpr int NB = ND + 1;             // barred fields: x-bar, v-bar_1..ND
    constexpr int NQ = ND == 3 ? 6 : 3;
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

    const float *bar[NB];
    bar[0] = a.xb;
#pragma unroll
    for (int c = 0; c < ND; ++c) bar[1 + c] = a.vb[c];

    float cur[NB][RY + 1], nxt[NB][RY + 1];
#pragma unroll
    for (int A = 0; A < NB; ++A)
#pragma unroll
        for (int q = 0; q <= RY; ++q) cur[A][q] = io.ld(bar[A] + sz * zc0, xo, rowoff(q));

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_next = t < dz - 1;
        if (ND == 3) {
            const size_t pn = sz * min(t + 1, dz - 1);
#pragma unroll
            for (int A = 0; A < NB; ++A)
#pragma unroll
                for (int q = 0; q <= RY; ++q) nxt[A][q] = io.ld(bar[A] + pn, xo, rowoff(q));
        }
        float P[ND][RY], Q[NQ][RY];
#pragma unroll
        for (int c = 0; c < ND; ++c)
#pragma unroll
            for (int r = 0; r < RY; ++r) P[c][r] = io.ld(a.p[c] + sz * t, xo, rowoff(r));
#pragma unroll
        for (int k = 0; k < NQ; ++k)
#pragma unroll
            for (int r = 0; r < RY; ++r) Q[k][r] = io.ld(a.q[k] + sz * t, xo, rowoff(r));

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_next = y0 + r < dy - 1;
            // F[A][d] = F_d of barred field A: a[i + e_d] - a[i], exactly 0 on the last index of the axis
            float F[NB][3];
#pragma unroll
            for (int A = 0; A < NB; ++A) {
                const float c = cur[A][r];
                const float cx = wave_next(c);
                F[A][0] = x_next ? cx - c : 0.0f;
                F[A][1] = y_next ? cur[A][r + 1] - c : 0.0f;
                F[A][2] = (ND == 3 && z_next) ? nxt[A][r] - c : 0.0f;
            }
            // P_d += sigma_P (F_d(x-bar) - v-bar_d);  P /= max(1, |P| / r1)
#pragma unroll
            for (int d = 0; d < ND; ++d) P[d][r] = P[d][r] + a.sigma_p * (F[0][d] - cur[1 + d][r]);
            {
                float s = P[0][r] * P[0][r] + P[1][r] * P[1][r];
                if (ND == 3) s = s + P[ND - 1][r] * P[ND - 1][r];
                const float n = sqrtf(s) / a.r1;
                const float den = n > 1.0f ? n : 1.0f;   // p / 1 is p: the same bits as leaving it alone
#pragma unroll
                for (int d = 0; d < ND; ++d) P[d][r] = P[d][r] / den;
            }
            // Q += sigma_Q E(v-bar) (symmetrised forward differences);  Q /= max(1, |Q|_F / r0)
            Q[GQ11][r] = Q[GQ11][r] + a.sigma_q * F[1][0];
            Q[GQ22][r] = Q[GQ22][r] + a.sigma_q * F[2][1];
            Q[GQ12][r] = Q[GQ12][r] + a.sigma_q * (0.5f * (F[1][1] + F[2][0]));
            float sd = Q[GQ11][r] * Q[GQ11][r] + Q[GQ22][r] * Q[GQ22][r];
            float so = Q[GQ12][r] * Q[GQ12][r];
            if constexpr (ND == 3) {
                Q[GQ33][r] = Q[GQ33][r] + a.sigma_q * F[3][2];
                Q[GQ13][r] = Q[GQ13][r] + a.sigma_q * (0.5f * (F[1][2] + F[3][0]));
                Q[GQ23][r] = Q[GQ23][r] + a.sigma_q * (0.5f * (F[2][2] + F[3][1]));
                sd = sd + Q[GQ33][r] * Q[GQ33][r];
                so = (so + Q[GQ13][r] * Q[GQ13][r]) + Q[GQ23][r] * Q[GQ23][r];
            }
            const float m = sqrtf(sd + 2.0f * so) / a.r0;
            const float den = m > 1.0f ? m : 1.0f;
#pragma unroll
            for (int k = 0; k < NQ; ++k) Q[k][r] = Q[k][r] / den;
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) {
#pragma unroll
                for (int c = 0; c < ND; ++c) io.st(a.p[c] + sz * t, xo, rowoff(r), P[c][r]);
#pragma unroll
                for (int k = 0; k < NQ; ++k) io.st(a.q[k] + sz * t, xo, rowoff(r), Q[k][r]);
            }
        }
        if (ND == 3) {
#pragma unroll
            for (int A = 0; A < NB; ++A)
#pragma unroll
                for (int q = 0; q <= RY; ++q) cur[A][q] = nxt[A][q];
        }
    }
}

struct TgvPrimalArgs {
    float *x, *xb;           // x (the caller's volume), x-bar
    const float *g;          // A^T y
    float *v[3], *vb[3];
    const float *p[3], *q[6];
    int dx, dy, dz;
    float tau_v;
};

// The mirror image of the dual march: the -x neighbour is the previous lane (lane 0 of a wave is the halo lane), the -y
// neighbour the previous register (one halo row above the tile, only for the four fields that are differenced along y),
// the -z neighbour the carried registers of the plane before (the four fields that are differenced along z; a z-chunk
// loads them once for the plane below its first).  P and Q are read once per launch (plus halos) and not written; x, g, v
// (and the step field of an Update::STEP_ARRAY functor) are read and x, x-bar, v, v-bar written at the lane's own voxels.
// amdgpu_waves_per_eu: the step field's registers must not cost a wave of the 5 (3D) and 8 (2D) that tgv_primal_kernel runs per SIMD.
template <int ND, class Update, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) __attribute__((amdgpu_waves_per_eu(ND == 3 ? 5 : 8))) void pdhg_tgv_primal_march(TgvPrimalArgs a, Update update, int gx, int gy,
                                                                     int tiles_per_xcd, int zchunk)
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

    // the plane below: P3, Q33, Q13, Q23
    float Zp[4][RY];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < RY; ++r) Zp[k][r] = 0.0f;
    if (ND == 3 && zc0 > 0) {
        const size_t pb = sz * (zc0 - 1);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            Zp[0][r] = io.ld(a.p[ND - 1] + pb, xo, rowoff(r + 1));
            Zp[1][r] = io.ld(a.q[GQ33] + pb, xo, rowoff(r + 1));
            Zp[2][r] = io.ld(a.q[GQ13] + pb, xo, rowoff(r + 1));
            Zp[3][r] = io.ld(a.q[GQ23] + pb, xo, rowoff(r + 1));
        }
    }

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_prev = t > 0;
        const size_t pt = sz * t;
        // rows -1..RY-1 (slot q) of the fields differenced along y, rows 0..RY-1 (slot r) of the others
        float P1[RY], P2[RY + 1], Q11[RY], Q22[RY + 1], Q12[RY + 1];
        float P3[RY], Q33[RY], Q13[RY], Q23[RY + 1];
        float X[RY], G[RY], T[RY], V[ND][RY];
#pragma unroll
        for (int q = 0; q <= RY; ++q) {
            P2[q] = io.ld(a.p[1] + pt, xo, rowoff(q));
            Q22[q] = io.ld(a.q[GQ22] + pt, xo, rowoff(q));
            Q12[q] = io.ld(a.q[GQ12] + pt, xo, rowoff(q));
            if (ND == 3) Q23[q] = io.ld(a.q[GQ23] + pt, xo, rowoff(q));
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            P1[r] = io.ld(a.p[0] + pt, xo, rowoff(r + 1));
            Q11[r] = io.ld(a.q[GQ11] + pt, xo, rowoff(r + 1));
            if (ND == 3) {
                P3[r] = io.ld(a.p[ND - 1] + pt, xo, rowoff(r + 1));
                Q33[r] = io.ld(a.q[GQ33] + pt, xo, rowoff(r + 1));
                Q13[r] = io.ld(a.q[GQ13] + pt, xo, rowoff(r + 1));
            }
            X[r] = io.ld(a.x + pt, xo, rowoff(r + 1));
            G[r] = io.ld(a.g + pt, xo, rowoff(r + 1));
            if constexpr (Update::STEP_ARRAY) T[r] = io.ld(update.step + pt, xo, rowoff(r + 1));
#pragma unroll
            for (int c = 0; c < ND; ++c) V[c][r] = io.ld(a.v[c] + pt, xo, rowoff(r + 1));
        }

        float Xn[RY], Xb[RY], Vn[ND][RY], Vb[ND][RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_prev = y0 + r > 0;
            // B_d(a)[i] = a[i] - a[i - e_d], a[i] itself on the first index of the axis
            auto bx = [&](float c) __attribute__((always_inline)) { const float l = wave_prev(c); return x_prev ? c - l : c; };
            auto by = [&](float c, float up) __attribute__((always_inline)) { return y_prev ? c - up : c; };
            auto bz = [&](float c, float below) __attribute__((always_inline)) { return z_prev ? c - below : c; };
            // x: div = (B_1 P1 + B_2 P2) + B_3 P3, then the update of tv_primal_march
            float div = bx(P1[r]) + by(P2[r + 1], P2[r]);
            if (ND == 3) div = div + bz(P3[r], Zp[0][r]);
            XS o;
            if constexpr (Update::STEP_ARRAY) o = update(X[r], G[r], div, T[r]);
            else o = update(X[r], G[r], div);
            Xn[r] = o.x;
            Xb[r] = o.s;
            // v: acc = P_d + B_d(Q_dd), then + B_e(Q_de) for e != d in ascending e
            float acc[3];
            acc[0] = (P1[r] + bx(Q11[r])) + by(Q12[r + 1], Q12[r]);
            acc[1] = (P2[r + 1] + by(Q22[r + 1], Q22[r])) + bx(Q12[r + 1]);
            if constexpr (ND == 3) {
                acc[0] = acc[0] + bz(Q13[r], Zp[2][r]);
                acc[1] = acc[1] + bz(Q23[r + 1], Zp[3][r]);
                acc[2] = ((P3[r] + bz(Q33[r], Zp[1][r])) + bx(Q13[r])) + by(Q23[r + 1], Q23[r]);
            }
#pragma unroll
            for (int c = 0; c < ND; ++c) {
                const float vn = V[c][r] + a.tau_v * acc[c];
                Vn[c][r] = vn;
                Vb[c][r] = (vn + vn) - V[c][r];
            }
            if constexpr (ND == 3) {
                Zp[0][r] = P3[r]; Zp[1][r] = Q33[r]; Zp[2][r] = Q13[r]; Zp[3][r] = Q23[r + 1];
            }
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) {
                io.st(a.x + pt, xo, rowoff(r + 1), Xn[r]);
                io.st(a.xb + pt, xo, rowoff(r + 1), Xb[r]);
#pragma unroll
                for (int c = 0; c < ND; ++c) {
                    io.st(a.v[c] + pt, xo, rowoff(r + 1), Vn[c][r]);
                    io.st(a.vb[c] + pt, xo, rowoff(r + 1), Vb[c][r]);
                }
            }
        }
    }
}

// The only launch sites of the two marches: TGV's tile, 4 rows per lane, 2 x 2 waves, 63 columns per wave.
template <int ND>
static int pdhg_tgv_dual_launch(const TgvDualArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "PDHG", a.dx, a.dy, a.dz, 63, 2, 2, 4, ND == 3)) return rc;
    pdhg_tgv_dual_march<ND, 4, 2, 2><<<(unsigned)g.blocks, 64 * 2 * 2, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

template <int ND, class Update>
static int pdhg_tgv_primal_launch(const TgvPrimalArgs &a, Update update, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "PDHG", a.dx, a.dy, a.dz, 63, 2, 2, 4, ND == 3)) return rc;
    pdhg_tgv_primal_march<ND, Update, 4, 2, 2><<<(unsigned)g.blocks, 64 * 2 * 2, 0, st>>>(a, update, g.gx, g.gy, g.tiles_per_xcd,
                                                                                        g.zchunk);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}
