// TGV dual launch (steps 1-2 of an iteration, docs/kernels/tgv.md): P and Q ascend along the forward differences of the
// barred primal fields and are projected onto their balls, in place.  Included inside the anonymous namespace of
// tgv_kernels.hip (uses TgvArgs; PlaneIO, wave_next of zmarch_common.h, the Q index names).
//
// z-march on the skeleton of rof_zmarch.inl: a lane owns RY rows of one x column and walks z.  The +x neighbour is the next
// lane (lane 63 of a wave is a halo lane: 63 columns per wave), the +y neighbour the next register (one halo row below the
// tile), the +z neighbour the plane loaded one step ahead, which becomes the current plane of the next step: U-bar and
// V-bar are read once per launch (plus halos), P and Q read and written once.  The launch reads only fields it does not
// write (U-bar, V-bar) at neighbouring voxels, so it needs no second copy of anything and no warm-up plane.
template <int ND, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void tgv_dual_kernel(TgvArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
{
    constexpr int NB = ND + 1;             // barred fields: U-bar, V-bar_1..ND
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
    bar[0] = a.ub;
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
            // step 1: P_d += sigma (F_d(U-bar) - V-bar_d);  P /= max(1, |P| / alpha1)
#pragma unroll
            for (int d = 0; d < ND; ++d) P[d][r] = P[d][r] + a.sigma * (F[0][d] - cur[1 + d][r]);
            {
                float s = P[0][r] * P[0][r] + P[1][r] * P[1][r];
                if (ND == 3) s = s + P[ND - 1][r] * P[ND - 1][r];
                const float n = sqrtf(s) / a.alpha1;
                const float den = n > 1.0f ? n : 1.0f;   // p / 1 is p: the same bits as leaving it alone
#pragma unroll
                for (int d = 0; d < ND; ++d) P[d][r] = P[d][r] / den;
            }
            // step 2: Q += sigma E(V-bar) (symmetrised forward differences);  Q /= max(1, |Q|_F / alpha0)
            Q[TQ11][r] = Q[TQ11][r] + a.sigma * F[1][0];
            Q[TQ22][r] = Q[TQ22][r] + a.sigma * F[2][1];
            Q[TQ12][r] = Q[TQ12][r] + a.sigma * (0.5f * (F[1][1] + F[2][0]));
            float sd = Q[TQ11][r] * Q[TQ11][r] + Q[TQ22][r] * Q[TQ22][r];
            float so = Q[TQ12][r] * Q[TQ12][r];
            if constexpr (ND == 3) {
                Q[TQ33][r] = Q[TQ33][r] + a.sigma * F[3][2];
                Q[TQ13][r] = Q[TQ13][r] + a.sigma * (0.5f * (F[1][2] + F[3][0]));
                Q[TQ23][r] = Q[TQ23][r] + a.sigma * (0.5f * (F[2][2] + F[3][1]));
                sd = sd + Q[TQ33][r] * Q[TQ33][r];
                so = (so + Q[TQ13][r] * Q[TQ13][r]) + Q[TQ23][r] * Q[TQ23][r];
            }
            const float m = sqrtf(sd + 2.0f * so) / a.alpha0;
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

template <int ND, int RY, int WX, int WY>
static int tgv_dual_launch(const TgvArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "TGV", a.dx, a.dy, a.dz, 63, WX, WY, RY, ND == 3)) return rc;
    tgv_dual_kernel<ND, RY, WX, WY><<<(unsigned)g.blocks, 64 * WX * WY, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}
