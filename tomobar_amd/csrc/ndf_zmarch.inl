// One NDF iteration as a register-blocked z-march (docs/kernels/ndf.md).  Included inside the anonymous namespace of
// ndf_kernels.hip (uses NdfArgs; PlaneIO, wave_prev, wave_next of zmarch_common.h, the NDF_* penalty names).
//
// A lane owns RY rows of one x column and walks z.  The flux of a voxel's three FORWARD differences is evaluated once; the
// flux of a backward difference is the neighbour's forward flux with the sign turned -- the three penalties are odd
// functions and every operation in them rounds symmetrically, so g(U[i - e] - c) has the bits of -g(c - U[i - e]) -- except
// that a zero difference gives +0 both ways and Tukey's rejected range gives +0 both ways (ndf_flux returns that second
// value, `gn`, beside g).  So:
//   x  the +x value is the next lane's (lane 63 of a wave is a halo lane), the -x flux the previous lane's (lane 0 is a
//      halo lane): 62 columns per wave, both by DPP wave shifts;
//   y  the lane's registers plus one halo row above (its forward flux is evaluated too) and one below;
//   z  the plane loaded one step ahead becomes the current plane of the next step, the -z flux is carried from the step
//      before; a z-chunk evaluates it once from the seam plane below its first.
// Every plane of U is loaded once per z-chunk (plus the two seam planes and the halo rows / lanes), f once, U' written
// once: 12 B per voxel, algorithmic.
template <int PEN>
__device__ __forceinline__ void ndf_flux(float t, float sigma, float &g, float &gn)
{
    const bool in = fabsf(t) <= sigma;
    if (PEN == NDF_HUBER) {
        const float q = t / sigma;
        g = in ? q : copysignf(1.0f, t);
    } else if (PEN == NDF_PM) {
        const float r = t / sigma;
        g = t / (1.0f + r * r);
    } else {
        const float r = t / sigma;
        const float w = 1.0f - r * r;
        g = in ? t * (w * w) : 0.0f;
    }
    gn = (t == 0.0f || (PEN == NDF_TUKEY && !in)) ? 0.0f : -g;
}

template <int ND, int PEN, int RY, int WX, int WY>
__global__ __launch_bounds__(64 * WX * WY) void ndf_zmarch_kernel(NdfArgs a, int gx, int gy, int tiles_per_xcd, int zchunk)
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
    const int x = (xb * WX + (wave % WX)) * 62 - 1 + lane;
    const int y0 = (yb * WY + (wave / WX)) * RY;
    const int dx = a.dx, dy = a.dy, planes = a.planes;
    const int zc0 = a.out_begin + chunk * zchunk;
    const int zc1 = min(zc0 + zchunk, a.out_end);
    if (zc0 >= zc1) return;

    const size_t sz = (size_t)dx * dy;
    const bool emit_lane = (lane > 0) && (lane < 63) && (x < dx);
    const bool x_prev = x > 0, x_next = x < dx - 1;
    const unsigned xo = (unsigned)min(max(x, 0), dx - 1) * 4u;   // the clamped column: every load stays inside the plane
    const int wy0 = __builtin_amdgcn_readfirstlane(y0);
    const int pitch = dx * 4;
    const PlaneIO io{(int)(sz * 4)};
    // slot q = row y0 - 1 + q (q = 0 and q = RY + 1: the halo rows), clamped into the plane
    auto rowoff = [&](int q) __attribute__((always_inline)) { return min(max(wy0 - 1 + q, 0), dy - 1) * pitch; };
    const float sigma = a.sigma;

    float cur[RY + 2], nxt[RY + 2], gnz[RY];
#pragma unroll
    for (int q = 0; q <= RY + 1; ++q) cur[q] = io.ld(a.u_in + sz * zc0, xo, rowoff(q));
#pragma unroll
    for (int r = 0; r < RY; ++r) gnz[r] = 0.0f;
    if (ND == 3 && zc0 > 0) {
        // the seam below the chunk: the -z flux of the first plane comes from the forward difference of the plane before it
        const size_t pb = sz * (zc0 - 1);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            float g;
            ndf_flux<PEN>(cur[r + 1] - io.ld(a.u_in + pb, xo, rowoff(r + 1)), sigma, g, gnz[r]);
        }
    }

    for (int t = zc0; t < zc1; ++t) {
        __syncthreads();  // lockstep: the waves of a workgroup stay on the same plane
        const bool z_prev = t > 0, z_next = t < planes - 1;
        const size_t pt = sz * t;
        if (ND == 3) {
            const size_t pn = sz * min(t + 1, planes - 1);
#pragma unroll
            for (int q = 0; q <= RY + 1; ++q) nxt[q] = io.ld(a.u_in + pn, xo, rowoff(q));
        }
        float In[RY], Un[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) In[r] = io.ld(a.f + pt, xo, rowoff(r + 1));

        // the -y flux of the tile's first row: the forward flux of the halo row above it
        float g_up, gny;
        ndf_flux<PEN>(cur[1] - cur[0], sigma, g_up, gny);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool y_prev = y0 + r > 0, y_next = y0 + r < dy - 1;
            const float c = cur[r + 1];
            const float cx = wave_next(c);
            float g1, gn1, g2, gn2;
            ndf_flux<PEN>(x_next ? cx - c : 0.0f, sigma, g1, gn1);
            ndf_flux<PEN>(y_next ? cur[r + 2] - c : 0.0f, sigma, g2, gn2);
            const float m1 = wave_prev(gn1);
            float S = ((g1 + (x_prev ? m1 : 0.0f)) + g2) + (y_prev ? gny : 0.0f);
            gny = gn2;
            if (ND == 3) {
                float g3, gn3;
                ndf_flux<PEN>(z_next ? nxt[r + 1] - c : 0.0f, sigma, g3, gn3);
                S = (S + g3) + (z_prev ? gnz[r] : 0.0f);
                gnz[r] = gn3;
            }
            Un[r] = c + a.tau * (a.lambda * S - (c - In[r]));
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (emit_lane && y0 + r < dy) io.st(a.u_out + pt, xo, rowoff(r + 1), Un[r]);
        }
        if (ND == 3) {
#pragma unroll
            for (int q = 0; q <= RY + 1; ++q) cur[q] = nxt[q];
        }
    }
}

template <int ND, int PEN, int RY, int WX, int WY>
static int ndf_zmarch_launch(const NdfArgs &a, hipStream_t st)
{
    ZmarchGrid g;
    if (int rc = zmarch_grid(g, "NDF", a.dx, a.dy, a.out_end - a.out_begin, 62, WX, WY, RY, ND == 3)) return rc;
    ndf_zmarch_kernel<ND, PEN, RY, WX, WY><<<(unsigned)g.blocks, 64 * WX * WY, 0, st>>>(a, g.gx, g.gy, g.tiles_per_xcd, g.zchunk);
    return TOMO_OK;
}
