// Wavelet shrinkage for gfx950: W_t(X) = three levels of the 2D orthonormal Daubechies-5 transform of every (y, x) slice in
// periodization mode, soft threshold t on every detail coefficient, inverse transform.  The `_WAVELETS` suffix of a
// regularisation method averages it with the method's own prox (regularisersCuPy.prox_regul).  The reference names the
// suffix in its tutorials (docs/source/tutorials/regul_iter_recon.rst:113) but its tree holds no implementation (the step
// lived in the removed RecToolsIR class, on the CUDA-only pypwt package): what is computed is the algorithm stated in
// docs/kernels/wavelets.md, formula-level parity, unpinned -- tests/_wavelet_oracle.py restates it in numpy and these
// kernels reproduce its float32 form bit for bit (one rounding per product and per sum in the stated order:
// -ffp-contract=off and no fmaf here).
//
// Six launches per call, one forward and one inverse per level, over all slices (grid z).  A forward workgroup stages a
// tile of its input with the circular apron of 8 samples per axis in LDS, filters x and then y out of LDS and writes the
// four sub-band tiles, the three detail bands already thresholded; an inverse workgroup stages the four sub-band tiles with
// their apron of 4 coefficients per axis, undoes y and then x and writes the approximation of the level above (level 1:
// the output, averaged with `mix` where one is given).  Nothing but the pyramid goes through memory: no row-filtered
// intermediate, no threshold pass, no mixing pass.
//
// The pyramid of one slice: for level l = 1, 2, 3 (n_0 = n, n_l = ceil(n_{l-1} / 2)) the bands LL, LH, HL, HH of
// ny_l x nx_l floats each, in that order, levels in ascending order; the first letter is the x filter, the second the y
// filter (LH = low-pass along x, high-pass along y).  The pyramids of the slices follow each other.  LL_1 and LL_2
// are work space: the forward pass leaves the approximations there, the inverse pass overwrites them with its own.
#include "tomo_common.h"

namespace {

// the db5 scaling filter h (natural order) and the wavelet filter g[k] = (-1)^k h[9 - k]: float32 roundings of the float64
// literals of docs/kernels/wavelets.md (tests/test_wavelet_oracle.py derives them from the Daubechies polynomial)
#define WL_H0 0.16010239797419293f
#define WL_H1 0.6038292697971896f
#define WL_H2 0.7243085284377733f
#define WL_H3 0.1384281459013205f
#define WL_H4 -0.242294887066382f
#define WL_H5 -0.03224486958463838f
#define WL_H6 0.0775714938400457f
#define WL_H7 -0.006241490212798274f
#define WL_H8 -0.012580751999082002f
#define WL_H9 0.0033357252854737717f
__device__ constexpr float WL_H[10] = {WL_H0, WL_H1, WL_H2, WL_H3, WL_H4, WL_H5, WL_H6, WL_H7, WL_H8, WL_H9};
__device__ constexpr float WL_G[10] = {WL_H9, -(WL_H8), WL_H7, -(WL_H6), WL_H5, -(WL_H4), WL_H3, -(WL_H2), WL_H1, -(WL_H0)};

constexpr int WL_LEVELS = 3;
constexpr int WL_T = 32;               // a tile: WL_T x WL_T coefficients per band = 2 WL_T x 2 WL_T samples
constexpr int WL_THREADS = 256;
constexpr int WL_FIN = 2 * WL_T + 8;   // forward: staged samples per axis (apron 8)
constexpr int WL_ICO = WL_T + 4;       // inverse: staged coefficients per axis (apron 4)

__device__ __forceinline__ float wl_soft(float d, float t)
{
    const float v = fabsf(d) - t;
    return copysignf(v > 0.0f ? v : 0.0f, d);
}

// index of sample `v` (any integer >= -n_e) of the periodised, even-extended line of n samples in the line itself
__device__ __forceinline__ int wl_wrap_sample(int v, int n, int n_e)
{
    v %= n_e;
    if (v < 0) v += n_e;
    return v < n ? v : n - 1;   // the duplicated last sample of an odd line
}

// One level forward.  in: slices of ny x nx samples, rows `pitch` apart, slices `in_slice` apart.  bands: LL of this level
// (LH, HL, HH follow at my * mx each), slices `pyr_slice` apart.  my = ceil(ny / 2), mx = ceil(nx / 2).
__global__ __launch_bounds__(WL_THREADS) void wl_forward_level(const float *__restrict__ in, size_t in_slice, int pitch, int ny, int nx,
                                                               float *__restrict__ bands, size_t pyr_slice, int my, int mx,
                                                               float t, int slices)
{
    __shared__ __attribute__((aligned(16))) float s_in[WL_FIN][WL_FIN];
    __shared__ float s_lo[WL_FIN][WL_T], s_hi[WL_FIN][WL_T];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * WL_T, j0 = blockIdx.x * WL_T;   // first coefficient of the tile
    const int ny_e = 2 * my, nx_e = 2 * mx;
    const size_t band = (size_t)my * mx;

    for (int z = blockIdx.z; z < slices; z += gridDim.z) {
        const float *src = in + (size_t)z * in_slice;
        for (int idx = tid; idx < WL_FIN * WL_FIN; idx += WL_THREADS) {
            const int rr = idx / WL_FIN, cc = idx - rr * WL_FIN;
            const int gy = wl_wrap_sample(2 * i0 + rr, ny, ny_e), gx = wl_wrap_sample(2 * j0 + cc, nx, nx_e);
            s_in[rr][cc] = src[(size_t)gy * pitch + gx];
        }
        __syncthreads();

        // x: a[j] = sum_k h[k] x[2 j + k], d[j] likewise with g, for every staged row
        for (int idx = tid; idx < WL_FIN * WL_T; idx += WL_THREADS) {
            const int rr = idx / WL_T, j = idx - rr * WL_T;
            const float2 *row = reinterpret_cast<const float2 *>(&s_in[rr][2 * j]);
            float a = 0.0f, d = 0.0f;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float2 v = row[q];
                a = a + WL_H[2 * q] * v.x;
                d = d + WL_G[2 * q] * v.x;
                a = a + WL_H[2 * q + 1] * v.y;
                d = d + WL_G[2 * q + 1] * v.y;
            }
            s_lo[rr][j] = a;
            s_hi[rr][j] = d;
        }
        __syncthreads();

        // y, then the threshold on the three detail bands
        float *dst = bands + (size_t)z * pyr_slice;
        for (int idx = tid; idx < WL_T * WL_T; idx += WL_THREADS) {
            const int i = idx / WL_T, j = idx - i * WL_T;
            if (i0 + i >= my || j0 + j >= mx) continue;
            float ll = 0.0f, lh = 0.0f, hl = 0.0f, hh = 0.0f;
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const float lo = s_lo[2 * i + k][j], hi = s_hi[2 * i + k][j];
                ll = ll + WL_H[k] * lo;
                lh = lh + WL_G[k] * lo;
                hl = hl + WL_H[k] * hi;
                hh = hh + WL_G[k] * hi;
            }
            const size_t o = (size_t)(i0 + i) * mx + (j0 + j);
            dst[o] = ll;
            dst[band + o] = wl_soft(lh, t);
            dst[2 * band + o] = wl_soft(hl, t);
            dst[3 * band + o] = wl_soft(hh, t);
        }
        __syncthreads();   // the next slice restages s_in, s_lo and s_hi
    }
}

// One level inverse.  bands as in wl_forward_level (read); out: slices of ny x nx samples (ny in {2 my - 1, 2 my}, nx
// likewise), rows `pitch` apart, slices `out_slice` apart.  mix (or null): an array laid out like `out`, read at the index
// written (once, so a one-touch stream: non-temporal); it may be `out` itself.
__global__ __launch_bounds__(WL_THREADS) void wl_inverse_level(const float *__restrict__ bands, size_t pyr_slice, int my, int mx,
                                                               float *out, size_t out_slice, int pitch, int ny, int nx,
                                                               const float *mix, int slices)
{
    __shared__ float s_c[4][WL_ICO][WL_ICO];        // LL, LH, HL, HH with the apron of 4 below
    __shared__ float s_l[2 * WL_T][WL_ICO], s_h[2 * WL_T][WL_ICO];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.y * WL_T, q0 = blockIdx.x * WL_T;   // first coefficient whose sample pair the tile writes
    const size_t band = (size_t)my * mx;

    for (int z = blockIdx.z; z < slices; z += gridDim.z) {
        const float *src = bands + (size_t)z * pyr_slice;
        for (int idx = tid; idx < WL_ICO * WL_ICO; idx += WL_THREADS) {
            const int rr = idx / WL_ICO, cc = idx - rr * WL_ICO;
            int gi = (p0 - 4 + rr) % my, gj = (q0 - 4 + cc) % mx;
            if (gi < 0) gi += my;
            if (gj < 0) gj += mx;
            const size_t o = (size_t)gi * mx + gj;
            s_c[0][rr][cc] = src[o];
            s_c[1][rr][cc] = src[band + o];
            s_c[2][rr][cc] = src[2 * band + o];
            s_c[3][rr][cc] = src[3 * band + o];
        }
        __syncthreads();

        // y: rows 2 p (taps k = 0, 2, .., 8) and 2 p + 1 (k = 1, 3, .., 9) from the coefficient rows p, p - 1, .., p - 4
        for (int idx = tid; idx < WL_T * WL_ICO; idx += WL_THREADS) {
            const int p = idx / WL_ICO, c = idx - p * WL_ICO;
            float le = 0.0f, lo = 0.0f, he = 0.0f, ho = 0.0f;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float ll = s_c[0][p + 4 - q][c], lh = s_c[1][p + 4 - q][c];
                const float hl = s_c[2][p + 4 - q][c], hh = s_c[3][p + 4 - q][c];
                le = le + WL_H[2 * q] * ll;
                le = le + WL_G[2 * q] * lh;
                lo = lo + WL_H[2 * q + 1] * ll;
                lo = lo + WL_G[2 * q + 1] * lh;
                he = he + WL_H[2 * q] * hl;
                he = he + WL_G[2 * q] * hh;
                ho = ho + WL_H[2 * q + 1] * hl;
                ho = ho + WL_G[2 * q + 1] * hh;
            }
            s_l[2 * p][c] = le;
            s_l[2 * p + 1][c] = lo;
            s_h[2 * p][c] = he;
            s_h[2 * p + 1][c] = ho;
        }
        __syncthreads();

        // x: samples 2 q and 2 q + 1 of every row
        float *dst = out + (size_t)z * out_slice;
        const float *mx_src = mix ? mix + (size_t)z * out_slice : nullptr;
        for (int idx = tid; idx < 2 * WL_T * WL_T; idx += WL_THREADS) {
            const int r = idx / WL_T, q = idx - r * WL_T;
            const int gy = 2 * p0 + r, gx = 2 * (q0 + q);
            if (gy >= ny || gx >= nx) continue;
            float e = 0.0f, o = 0.0f;
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const float a = s_l[r][q + 4 - s], d = s_h[r][q + 4 - s];
                e = e + WL_H[2 * s] * a;
                e = e + WL_G[2 * s] * d;
                o = o + WL_H[2 * s + 1] * a;
                o = o + WL_G[2 * s + 1] * d;
            }
            const size_t at = (size_t)gy * pitch + gx;
            if (mx_src) {
                dst[at] = (__builtin_nontemporal_load(mx_src + at) + e) * 0.5f;
                if (gx + 1 < nx) dst[at + 1] = (__builtin_nontemporal_load(mx_src + at + 1) + o) * 0.5f;
            } else {
                dst[at] = e;
                if (gx + 1 < nx) dst[at + 1] = o;
            }
        }
        __syncthreads();   // the next slice restages s_c, s_l and s_h
    }
}

// ---- host: the geometry of the pyramid
struct WlGeom {
    int ny[WL_LEVELS + 1], nx[WL_LEVELS + 1];   // [0]: the slice, [l]: the bands of level l
    size_t off[WL_LEVELS + 1];                  // [l]: where level l starts in a slice's pyramid (l = 1 ..), floats
    size_t floats;                              // per slice
    int slices;
};

static WlGeom wl_geom(int dx, int dy, int dz, int nd)
{
    WlGeom g;
    g.ny[0] = dy;
    g.nx[0] = dx;
    g.slices = nd == 2 ? 1 : dz;
    g.off[0] = 0;
    size_t at = 0;
    for (int l = 1; l <= WL_LEVELS; ++l) {
        g.ny[l] = (g.ny[l - 1] + 1) / 2;
        g.nx[l] = (g.nx[l - 1] + 1) / 2;
        g.off[l] = at;
        at += 4 * (size_t)g.ny[l] * g.nx[l];
    }
    g.floats = at;
    return g;
}

static int wl_check(const char *op, int device, int dx, int dy, int dz, int nd)
{
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");
    TOMO_REQUIRE(nd == 2 || nd == 3, "2D or 3D arrays must be provided only");
    TOMO_REQUIRE(dx >= 1 && dy >= 1 && (nd == 2 || dz >= 1), "%s needs every dimension >= 1", op);
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 30), "%s: a slice of %d x %d is too large", op, dx, dy);
    return TOMO_OK;
}

static dim3 wl_grid(int my, int mx, int slices)
{
    return dim3((unsigned)ceil_div(mx, WL_T), (unsigned)ceil_div(my, WL_T), (unsigned)(slices < 65535 ? slices : 65535));
}

// the three forward launches: in -> pyr
static int wl_forward(const WlGeom &g, const float *in, float *pyr, float t, hipStream_t st)
{
    for (int l = 1; l <= WL_LEVELS; ++l) {
        const float *src = l == 1 ? in : pyr + g.off[l - 1];   // LL of the level above
        const size_t src_slice = l == 1 ? (size_t)g.ny[0] * g.nx[0] : g.floats;
        hipLaunchKernelGGL(wl_forward_level, wl_grid(g.ny[l], g.nx[l], g.slices), dim3(WL_THREADS), 0, st, src, src_slice,
                           g.nx[l - 1], g.ny[l - 1], g.nx[l - 1], pyr + g.off[l], g.floats, g.ny[l], g.nx[l], t, g.slices);
        TOMO_LAUNCH_CHECK();
    }
    return TOMO_OK;
}

// the three inverse launches: pyr -> out (LL_2 and LL_1 of pyr are overwritten on the way)
static int wl_inverse(const WlGeom &g, float *pyr, float *out, const float *mix, hipStream_t st)
{
    for (int l = WL_LEVELS; l >= 1; --l) {
        float *dst = l == 1 ? out : pyr + g.off[l - 1];
        const size_t dst_slice = l == 1 ? (size_t)g.ny[0] * g.nx[0] : g.floats;
        hipLaunchKernelGGL(wl_inverse_level, wl_grid(g.ny[l], g.nx[l], g.slices), dim3(WL_THREADS), 0, st, pyr + g.off[l], g.floats,
                           g.ny[l], g.nx[l], dst, dst_slice, g.nx[l - 1], g.ny[l - 1], g.nx[l - 1], l == 1 ? mix : nullptr, g.slices);
        TOMO_LAUNCH_CHECK();
    }
    return TOMO_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_wavelet_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if ((nd != 2 && nd != 3) || dx < 1 || dy < 1 || (nd == 3 && dz < 1)) return 0;
    const WlGeom g = wl_geom(dx, dy, dz, nd);
    return g.floats * (size_t)g.slices * sizeof(float);
}

extern "C" int tomo_wavelet_forward(int device, const float *in_dev, float *pyramid_dev, int dx, int dy, int dz, int nd,
                                    float threshold, void *stream)
{
    int rc = wl_check("the wavelet transform", device, dx, dy, dz, nd);
    if (rc != TOMO_OK) return rc;
    TOMO_REQUIRE(threshold >= 0.0f, "the wavelet threshold must not be negative");
    TOMO_REQUIRE(in_dev && pyramid_dev, "NULL data pointer");
    TOMO_ON_DEVICE(device);
    return wl_forward(wl_geom(dx, dy, dz, nd), in_dev, pyramid_dev, threshold, as_stream(stream));
}

extern "C" int tomo_wavelet_inverse(int device, float *pyramid_dev, float *out_dev, const float *mix_dev, int dx, int dy, int dz,
                                    int nd, void *stream)
{
    int rc = wl_check("the wavelet transform", device, dx, dy, dz, nd);
    if (rc != TOMO_OK) return rc;
    TOMO_REQUIRE(pyramid_dev && out_dev, "NULL data pointer");
    TOMO_ON_DEVICE(device);
    return wl_inverse(wl_geom(dx, dy, dz, nd), pyramid_dev, out_dev, mix_dev, as_stream(stream));
}

extern "C" int tomo_wavelet_shrink(int device, const float *in_dev, float *out_dev, const float *mix_dev, int dx, int dy, int dz,
                                   int nd, float threshold, void *stream)
{
    int rc = wl_check("wavelet shrinkage", device, dx, dy, dz, nd);
    if (rc != TOMO_OK) return rc;
    TOMO_REQUIRE(threshold >= 0.0f, "the wavelet threshold must not be negative");
    TOMO_REQUIRE(in_dev && out_dev, "NULL data pointer");
    TOMO_ON_DEVICE(device);
    hipStream_t st = as_stream(stream);
    const WlGeom g = wl_geom(dx, dy, dz, nd);
    void *pyr = nullptr;
    rc = tomo_arena_get(device, st, ARENA_TV, g.floats * (size_t)g.slices * sizeof(float), &pyr, true);
    if (rc != TOMO_OK) return rc;
    rc = wl_forward(g, in_dev, (float *)pyr, threshold, st);
    if (rc != TOMO_OK) return rc;
    return wl_inverse(g, (float *)pyr, out_dev, mix_dev, st);
}
