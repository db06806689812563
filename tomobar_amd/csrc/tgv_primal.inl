// TGV primal launch (steps 3-4 of an iteration, docs/kernels/tgv.md): U and V descend along the backward differences
// (negative adjoints of the forward ones) of the new duals and are extrapolated into U-bar / V-bar, in place.  Included
// inside the anonymous namespace of tgv_kernels.hip (uses TgvArgs; PlaneIO, wave_prev of zmarch_common.h, the Q index names).
//
// The mirror image of tgv_dual.inl: the -x neighbour is the previous lane (lane 0 of a wave is the halo lane), the -y
// neighbour the previous register (one halo row above the tile, only for the four fields that are differenced along y),
// the -z neighbour the carried registers of the plane before (the four fields that are differenced along z; a z-chunk
// loads them once for the plane below its first).  P and Q are read once per launch (plus halos) and not written; U, V and
// the input are read and U, U-bar, V, V-bar written at the lane's own voxels only.
template <int ND, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void tgv_primal_kernel(TgvArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
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
            Zp[1][r] = io.ld(a.q[TQ33] + pb, xo, rowoff(r + 1));
            Zp[2][r] = io.ld(a.q[TQ13] + pb, xo, rowoff(r + 1));
            Zp[3][r] = io.ld(a.q[TQ23] + pb, xo, rowoff(r + 1));
        }
    }
    const float den = a.lambda + a.tau;

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_prev = t > 0;
        const size_t pt = sz * t;
        // rows -1..RY-1 (slot q) of the fields differenced along y, rows 0..RY-1 (slot r) of the others
        float P1[RY], P2[RY + 1], Q11[RY], Q22[RY + 1], Q12[RY + 1];
        float P3[RY], Q33[RY], Q13[RY], Q23[RY + 1];
        float U[RY], In[RY], V[ND][RY];
#pragma unroll
        for (int q = 0; q <= RY; ++q) {
            P2[q] = io.ld(a.p[1] + pt, xo, rowoff(q));
            Q22[q] = io.ld(a.q[TQ22] + pt, xo, rowoff(q));
            Q12[q] = io.ld(a.q[TQ12] + pt, xo, rowoff(q));
            if (ND == 3) Q23[q] = io.ld(a.q[TQ23] + pt, xo, rowoff(q));
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            P1[r] = io.ld(a.p[0] + pt, xo, rowoff(r + 1));
            Q11[r] = io.ld(a.q[TQ11] + pt, xo, rowoff(r + 1));
            if (ND == 3) {
                P3[r] = io.ld(a.p[ND - 1] + pt, xo, rowoff(r + 1));
                Q33[r] = io.ld(a.q[TQ33] + pt, xo, rowoff(r + 1));
                Q13[r] = io.ld(a.q[TQ13] + pt, xo, rowoff(r + 1));
            }
            U[r] = io.ld(a.u + pt, xo, rowoff(r + 1));
            In[r] = io.ld(a.f + pt, xo, rowoff(r + 1));
#pragma unroll
            for (int c = 0; c < ND; ++c) V[c][r] = io.ld(a.v[c] + pt, xo, rowoff(r + 1));
        }

        float Un[RY], Ub[RY], Vn[ND][RY], Vb[ND][RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_prev = y0 + r > 0;
            // B_d(a)[i] = a[i] - a[i - e_d], a[i] itself on the first index of the axis
            auto bx = [&](float c) __attribute__((always_inline)) { const float l = wave_prev(c); return x_prev ? c - l : c; };
            auto by = [&](float c, float up) __attribute__((always_inline)) { return y_prev ? c - up : c; };
            auto bz = [&](float c, float below) __attribute__((always_inline)) { return z_prev ? c - below : c; };
            // step 3
            float div = bx(P1[r]) + by(P2[r + 1], P2[r]);
            if (ND == 3) div = div + bz(P3[r], Zp[0][r]);
            const float un = (a.lambda * (U[r] + a.tau * div) + a.tau * In[r]) / den;
            Un[r] = un;
            Ub[r] = 2.0f * un - U[r];
            // step 4: acc = P_d + B_d(Q_dd), then + B_e(Q_de) for e != d in ascending e
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
                const float vn = V[c][r] + a.tau * acc[c];
                Vn[c][r] = vn;
                Vb[c][r] = 2.0f * vn - V[c][r];
            }
            if constexpr (ND == 3) {
                Zp[0][r] = P3[r]; Zp[1][r] = Q33[r]; Zp[2][r] = Q13[r]; Zp[3][r] = Q23[r + 1];
            }
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) {
                io.st(a.u + pt, xo, rowoff(r + 1), Un[r]);
                io.st(a.ub + pt, xo, rowoff(r + 1), Ub[r]);
#pragma unroll
                for (int c = 0; c < ND; ++c) {
                    io.st(a.v[c] + pt, xo, rowoff(r + 1), Vn[c][r]);
                    io.st(a.vb[c] + pt, xo, rowoff(r + 1), Vb[c][r]);
                }
            }
        }
    }
}

template <int ND, int RY, int WX, int WY>
static int tgv_primal_launch(const TgvArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "TGV", a.dx, a.dy, a.dz, 63, WX, WY, RY, ND == 3)) return rc;
    tgv_primal_kernel<ND, RY, WX, WY><<<(unsigned)g.blocks, 64 * WX * WY, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}
