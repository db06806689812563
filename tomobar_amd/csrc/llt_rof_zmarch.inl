// One LLT_ROF iteration as a register-blocked z-march, both stages fused (docs/kernels/llt_rof.md).  Included inside the
// anonymous namespace of llt_rof_kernels.hip (uses LrArgs; PlaneIO, wave_prev, wave_next of zmarch_common.h).
//
// A lane owns RY rows of one x column and walks z.  Stage 2 at a voxel needs the LLT flux E_d at i and i +- e_d and the ROF
// flux R_d at i and i - e_d; E_d needs U at radius 1 along d, R_d the norm n of the forward differences of all axes, so:
//   x  two halo lanes at each end of a wave (60 columns per wave): E1 on lanes 1..62 from U on lanes 0..63, R1 and n on
//      lanes 1..61; neighbours by DPP wave shifts;
//   y  E2 on the RY + 2 row slots y0 - 1 .. y0 + RY from U on RY + 4 (two halo rows each side, register neighbours); n and R2
//      on the RY + 1 row slots y0 - 1 .. y0 + RY - 1;
//   z  step t evaluates E3 of plane t + 1 once, from U of planes t, t + 1, t + 2, and carries E3 of planes t - 1 and t and R3
//      of plane t - 1 from the steps before; a z-chunk's prologue evaluates what its first output plane needs from the planes
//      below the seam.
// The six flux fields never go to memory: U and f are read once per voxel (plus halos and seam planes), U' written once --
// 12 B per voxel.
//
// Clamped indexing comes in two kinds (docs/kernels/diff4th.md).  Loads clamp column, row and plane into the array, so a
// lane, a row slot or a plane "outside" holds the value of the nearest one inside: that IS the specification's clamped
// neighbour of U.  E_d of an index outside the array is E_d of the nearest index inside -- not what an outside lane or row
// slot evaluates from its clamped U -- so stage 2 selects: the neighbour's E_d where the neighbour exists, the voxel's own
// otherwise; R_d of the missing backward neighbour is zero.  Both selections test against the faces of the array the launch
// addresses: a slab's ghost planes exist exactly where a z-neighbour does.

// E = h / (|h| + eps): the LLT flux of one axis
__device__ __forceinline__ float lr_sign_like(float h) { return h / (__builtin_fabsf(h) + 1e-8f); }

// E3 of one plane on the RY own rows (slots 2 .. RY + 1 of the RY + 4): zc = U of the plane, zm / zp = below / above it
template <int RY>
__device__ __forceinline__ void lr_e3(const float (&zm)[RY + 4], const float (&zc)[RY + 4], const float (&zp)[RY + 4], float (&E)[RY])
{
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const float c = zc[r + 2];
        E[r] = lr_sign_like((zp[r + 2] + zm[r + 2]) - (c + c));
    }
}

// R3 of one plane on the RY own rows: zc = U of the plane, zp = U of the plane above it (the seam prologue only; the march
// forms R3 with R1 and R2 from the one norm)
template <int RY>
__device__ __forceinline__ void lr_r3(const float (&zc)[RY + 4], const float (&zp)[RY + 4], float (&R)[RY])
{
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const float c = zc[r + 2];
        const float a1 = wave_next(c) - c, a2 = zc[r + 3] - c, a3 = zp[r + 2] - c;
        R[r] = a3 / sqrtf(((a1 * a1 + a2 * a2) + a3 * a3) + 1e-8f);
    }
}

template <int ND, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void lr_zmarch_kernel(LrArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
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
    const float eps = 1e-8f;

    // entering step t: ua = U(t), ub = U(t + 1) [clamped], E3m = E3(t - 1) [clamped], E3c = E3(t), R3m = R3(t - 1) or zero
    float ua[RY + 4], ub[RY + 4], uc[RY + 4];
    float E3m[RY], E3c[RY], E3n[RY], R3m[RY];
    if (ND == 3) {
        const int pm = max(zc0 - 1, 0);
        load_plane(uc, pm - 1);
        load_plane(ua, pm);
        load_plane(ub, pm + 1);
        lr_e3<RY>(uc, ua, ub, E3c);   // E3(pm): the plane below the chunk, or the first plane of the array
#pragma unroll
        for (int r = 0; r < RY; ++r) { E3m[r] = E3c[r]; R3m[r] = 0.0f; }
        if (zc0 > 0) {   // (wave-uniform) the chunk's first plane has a plane below it
            lr_r3<RY>(ua, ub, R3m);
            load_plane(uc, zc0 + 1);
            lr_e3<RY>(ua, ub, uc, E3c);
#pragma unroll
            for (int q = 0; q < RY + 4; ++q) { ua[q] = ub[q]; ub[q] = uc[q]; }
        }
    } else {
        load_plane(ua, 0);
    }

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const size_t pt = sz * t;
        float In[RY], Un[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) In[r] = io.ld(a.f + pt, xo, rowoff(r + 2));
        if (ND == 3) {
            if (t + 1 < planes) {   // (wave-uniform) E3 of the plane ahead, once
                load_plane(uc, t + 2);
                lr_e3<RY>(ua, ub, uc, E3n);
            } else {                // the last plane of the array: its +z neighbour is itself
#pragma unroll
                for (int r = 0; r < RY; ++r) E3n[r] = E3c[r];
            }
        }

        // E2 on the row slots y0 - 1 .. y0 + RY
        float E2[RY + 2];
#pragma unroll
        for (int w = 0; w < RY + 2; ++w) {
            const float c = ua[w + 1];
            E2[w] = lr_sign_like((ua[w + 2] + ua[w]) - (c + c));
        }

        // R2 of the row above the lane's first one
        float R2m;
        {
            const float c = ua[1];
            const float a1 = wave_next(c) - c, a2 = ua[2] - c;
            float s = a1 * a1 + a2 * a2;
            if (ND == 3) { const float a3 = ub[1] - c; s = s + a3 * a3; }
            R2m = a2 / sqrtf(s + eps);   // the first own row selects zero where the array has no row above it
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_prev = y0 + r > 0, y_next = y0 + r < dy - 1;
            const float c = ua[r + 2], cc = c + c;
            const float p1 = wave_next(c), m1 = wave_prev(c);
            const float a1 = p1 - c, a2 = ua[r + 3] - c;
            float a3 = 0.0f;
            float s = a1 * a1 + a2 * a2;
            if (ND == 3) { a3 = ub[r + 2] - c; s = s + a3 * a3; }
            const float n = sqrtf(s + eps);
            const float R1 = a1 / n, R2 = a2 / n;
            const float R1m = wave_prev(R1);
            const float v1 = R1 - (x_prev ? R1m : 0.0f);
            const float v2 = R2 - (y_prev ? R2m : 0.0f);
            R2m = R2;
            float V = v1 + v2;

            const float E1 = lr_sign_like((p1 + m1) - cc);
            const float e1p = wave_next(E1), e1m = wave_prev(E1);
            const float b1 = ((x_next ? e1p : E1) + (x_prev ? e1m : E1)) - (E1 + E1);
            const float Ey = E2[r + 1];
            const float b2 = ((y_next ? E2[r + 2] : Ey) + (y_prev ? E2[r] : Ey)) - (Ey + Ey);
            float B = b1 + b2;
            if (ND == 3) {
                const float R3 = a3 / n;
                V = V + (R3 - R3m[r]);
                R3m[r] = R3;
                B = B + ((E3n[r] + E3m[r]) - (E3c[r] + E3c[r]));
            }
            Un[r] = c - a.tau * ((a.lambda_llt * B - a.lambda_rof * V) + (c - In[r]));
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) io.st(a.u_out + pt, xo, rowoff(r + 2), Un[r]);
        }
        if (ND == 3) {
#pragma unroll
            for (int r = 0; r < RY; ++r) { E3m[r] = E3c[r]; E3c[r] = E3n[r]; }
#pragma unroll
            for (int q = 0; q < RY + 4; ++q) { ua[q] = ub[q]; ub[q] = uc[q]; }
        }
    }
}

template <int ND, int RY, int WX, int WY>
static int lr_zmarch_launch(const LrArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "LLT_ROF", a.dx, a.dy, a.out_end - a.out_begin, 60, WX, WY, RY, ND == 3)) return rc;
    lr_zmarch_kernel<ND, RY, WX, WY><<<(unsigned)g.blocks, 64 * WX * WY, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}
