// One Diff4th iteration as a register-blocked z-march, both stages fused (docs/kernels/diff4th.md).  Included inside the
// anonymous namespace of diff4th_kernels.hip (uses D4Args; PlaneIO, wave_prev, wave_next of zmarch_common.h).
//
// A lane owns RY rows of one x column and walks z.  Stage 2 at a voxel needs the weighted second derivative W at the six
// face neighbours, and W needs U at radius 1 (faces and the in-plane / cross-plane diagonals), so:
//   x  two halo lanes at each end of a wave (60 columns per wave): W is evaluated on lanes 1..62 from U on lanes 0..63,
//      neighbours by DPP wave shifts;
//   y  two halo rows above and below the tile: W on RY + 2 rows from U on RY + 4;
//   z  step t evaluates W of plane t + 1 once, from U of planes t, t + 1, t + 2 (registers), and carries W of planes t - 1
//      and t from the steps before; a z-chunk's prologue evaluates the two W planes its first output plane needs from the
//      planes below the seam.
// W never goes to memory: U and f are read once per voxel (plus halos and seam planes), U' written once -- 12 B per voxel.
//
// Clamped indexing comes in two kinds.  Loads clamp column, row and plane into the array, so a lane, a row slot or a plane
// "outside" holds the value of the nearest one inside: that IS the specification's clamped neighbour of U, and the
// differences a neighbouring lane or row slot forms from its own clamped values are the specification's too.  W of an
// index outside the array is W of the nearest index inside -- not what an outside lane or row slot evaluates from its
// clamped U -- so stage 2 selects: the neighbour's W where the neighbour exists, the voxel's own W otherwise.  In z the
// plane index itself is clamped before W is evaluated, which needs no select.
//
// The mixed derivatives reuse the central differences: with dy = U[y+1] - U[y-1] and dz = U[z+1] - U[z-1] formed once per
// lane and row slot (g2 = 0.5 dy and g3 = 0.5 dz are the same subtractions), k12 = 0.25 (dy[x+1] - dy[x-1]),
// k13 = 0.25 (dz[x+1] - dz[x-1]), k23 = 0.25 (dz[y+1] - dz[y-1]): the operands and the order of the specification.

// W of one plane on the RY + 2 row slots y0 - 1 .. y0 + RY.  zc = U of the plane (RY + 4 row slots y0 - 2 .. y0 + RY + 1),
// zm / zp = U of the planes below / above it (ND == 3 only).
template <int ND, int RY>
__device__ __forceinline__ void d4_weighted(const float (&zm)[RY + 4], const float (&zc)[RY + 4], const float (&zp)[RY + 4],
                                            float s2, float (&W)[RY + 2])
{
    float dz[RY + 4];
    if (ND == 3) {
#pragma unroll
        for (int q = 0; q < RY + 4; ++q) dz[q] = zp[q] - zm[q];
    }
#pragma unroll
    for (int w = 0; w < RY + 2; ++w) {
        const int u = w + 1;
        const float c = zc[u], cc = c + c;
        const float p1 = wave_next(c), m1 = wave_prev(c);
        const float g1 = 0.5f * (p1 - m1);
        const float h1 = (p1 + m1) - cc;
        const float p2 = zc[u + 1], m2 = zc[u - 1];
        const float dy = p2 - m2;
        const float g2 = 0.5f * dy;
        const float h2 = (p2 + m2) - cc;
        const float k12 = 0.25f * (wave_next(dy) - wave_prev(dy));
        float G = g1 * g1 + g2 * g2;
        float L = h1 + h2;
        float Q = (h1 * (g1 * g1) + h2 * (g2 * g2)) + 2.0f * ((g1 * g2) * k12);
        if (ND == 3) {
            const float g3 = 0.5f * dz[u];
            const float h3 = (zp[u] + zm[u]) - cc;
            const float k13 = 0.25f * (wave_next(dz[u]) - wave_prev(dz[u]));
            const float k23 = 0.25f * (dz[u + 1] - dz[u - 1]);
            G = G + g3 * g3;
            L = L + h3;
            Q = Q + ((h3 * (g3 * g3) + 2.0f * ((g1 * g3) * k13)) + 2.0f * ((g2 * g3) * k23));
        }
        // the second derivative along the gradient, Q / G where G > 0, else +0: the quotient is formed on every lane and
        // masked, so that no divergent branch is put round the division
        const float q = Q / (G > 0.0f ? G : 1.0f);
        const float eta = __builtin_bit_cast(float, __builtin_bit_cast(int, q) & (G > 0.0f ? -1 : 0));
        const float r = G / s2;
        const float cw = 1.0f / (1.0f + r);
        W[w] = (cw * cw) * eta + cw * (L - eta);
    }
}

template <int ND, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void d4_zmarch_kernel(D4Args a, int gx, int gy, int tiles_per_xcd, int zchunk)
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
    const int x = (xb * WX + (wave % WX)) * 60 - 2 + lane;
    const int y0 = (yb * WY + (wave / WX)) * RY;
    const int dx = a.dx, dy = a.dy, planes = a.planes;
    const int zc0 = a.out_begin + chunk * zchunk;
    const int zc1 = min(zc0 + zchunk, a.out_end);
    if (zc0 >= zc1) return;

    const size_t sz = (size_t)dx * dy;
    const bool emit_lane = (lane > 1) && (lane < 62) && (x < dx);
    const bool x_prev = x > 0, x_next = x < dx - 1;
    const unsigned xo = (unsigned)min(max(x, 0), dx - 1) * 4u;   // the clamped column: every load stays inside the plane
    const int wy0 = __builtin_amdgcn_readfirstlane(y0);
    const int pitch = dx * 4;
    const PlaneIO io{(int)(sz * 4)};
    // slot q = row y0 - 2 + q (q < 2 and q >= RY + 2: the halo rows), clamped into the plane
    auto rowoff = [&](int q) __attribute__((always_inline)) { return min(max(wy0 - 2 + q, 0), dy - 1) * pitch; };
    auto load_plane = [&](float (&dst)[RY + 4], int p) __attribute__((always_inline)) {
        const float *base = a.u_in + sz * (size_t)min(max(p, 0), planes - 1);   // the clamped plane
#pragma unroll
        for (int q = 0; q < RY + 4; ++q) dst[q] = io.ld(base, xo, rowoff(q));
    };
    const float s2 = a.sigma * a.sigma;

    // entering step t: ua = U(t), ub = U(t + 1) [clamped], Wm = W(t - 1) [clamped] on the own rows, Wc = W(t)
    float ua[RY + 4], ub[RY + 4], uc[RY + 4];
    float Wm[RY], Wc[RY + 2], Wn[RY + 2];
    if (ND == 3) {
        const int pm = max(zc0 - 1, 0);
        load_plane(uc, pm - 1);
        load_plane(ua, pm);
        load_plane(ub, pm + 1);
        d4_weighted<3, RY>(uc, ua, ub, s2, Wc);   // W(pm): the plane below the chunk, or the first plane of the array
#pragma unroll
        for (int r = 0; r < RY; ++r) Wm[r] = Wc[r + 1];
        if (zc0 > 0) {   // (wave-uniform) the chunk's first plane
            load_plane(uc, zc0 + 1);
            d4_weighted<3, RY>(ua, ub, uc, s2, Wc);
#pragma unroll
            for (int q = 0; q < RY + 4; ++q) { ua[q] = ub[q]; ub[q] = uc[q]; }
        }
    } else {
        load_plane(ua, 0);
        d4_weighted<2, RY>(ua, ua, ua, s2, Wc);
    }

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const size_t pt = sz * t;
        float In[RY], Un[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) In[r] = io.ld(a.f + pt, xo, rowoff(r + 2));
        if (ND == 3) {
            if (t + 1 < planes) {   // (wave-uniform) W of the plane ahead, once
                load_plane(uc, t + 2);
                d4_weighted<3, RY>(ua, ub, uc, s2, Wn);
            } else {                // the last plane of the array: its +z neighbour is itself
#pragma unroll
                for (int w = 0; w < RY + 2; ++w) Wn[w] = Wc[w];
            }
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_prev = y0 + r > 0, y_next = y0 + r < dy - 1;
            const float c = ua[r + 2];
            const float Wi = Wc[r + 1], W2 = Wi + Wi;
            const float wxp = wave_next(Wi), wxm = wave_prev(Wi);
            const float b1 = ((x_next ? wxp : Wi) + (x_prev ? wxm : Wi)) - W2;
            const float b2 = ((y_next ? Wc[r + 2] : Wi) + (y_prev ? Wc[r] : Wi)) - W2;
            float B = b1 + b2;
            if (ND == 3) B = B + ((Wn[r + 1] + Wm[r]) - W2);
            Un[r] = c - a.tau * (a.lambda * B + (c - In[r]));
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) io.st(a.u_out + pt, xo, rowoff(r + 2), Un[r]);
        }
        if (ND == 3) {
#pragma unroll
            for (int r = 0; r < RY; ++r) Wm[r] = Wc[r + 1];
#pragma unroll
            for (int w = 0; w < RY + 2; ++w) Wc[w] = Wn[w];
#pragma unroll
            for (int q = 0; q < RY + 4; ++q) { ua[q] = ub[q]; ub[q] = uc[q]; }
        }
    }
}

template <int ND, int RY, int WX, int WY>
static int d4_zmarch_launch(const D4Args &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "Diff4th", a.dx, a.dy, a.out_end - a.out_begin, 60, WX, WY, RY, ND == 3)) return rc;
    d4_zmarch_kernel<ND, RY, WX, WY><<<(unsigned)g.blocks, 64 * WX * WY, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}
