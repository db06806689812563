// Non-local total variation (NLTV) for gfx950: PatchSelect builds, for every pixel of every (y, x) slice, the table of its
// K most similar pixels inside a search window (indices H_i, H_j and weights W), and the NLTV iteration is a Jacobi sweep
// of the weighted non-local TV over those tables.  The reference's legacy demo (Demos/methods_IR_legacy/
// DemoFISTA_NLTV_2D.py) passes such tables under NLTV_H_i / NLTV_H_j / NLTV_Weights, but both halves lived in the
// regularisation toolkit it no longer depends on: what is computed is the algorithm stated in docs/kernels/nltv.md --
// formula-level parity, unpinned; tests/_nltv_oracle.py restates it in numpy and the kernels reproduce its float32 form bit
// for bit (one rounding per operation in the stated order, no FMA contraction: -ffp-contract=off and no fmaf here; / and
// sqrtf are the compiler's correctly rounded ones; the exponential is the specification's own polynomial, not expf).
//
// patch_select: one workgroup of 512 threads owns a 32 x 16 tile of one slice (slices along grid z).  The tile with an
// apron of S + P pixels is staged in LDS once; then, per search offset, the squared differences are filtered along x into
// an LDS row buffer (two buffers alternate, so one barrier per offset), every thread filters its pixel's column out of
// it and inserts the distance into its sorted list of K (key, offset id) pairs, which lives in registers: K is a template
// bound and the insertion a fully unrolled compare-and-shift with strict <, i.e. a stable order.  The key is the bit
// pattern of the distance (non-negative floats order like unsigned integers), so an empty slot (all ones) ranks behind
// every distance, +inf included.
//
// nltv_iter: one thread per pixel; the tables are read coalesced along x in their public layout [K][z][y][x], u is gathered
// through the cache.  Every index is clamped into the slice, so a corrupt table gives a wrong answer, never an access
// outside the array.  The iterations run under march_run of zmarch_common.h (ping-pong through one work array of the TV
// arena, the tolerance rule, the refusal of out == in).
#include "zmarch_common.h"

namespace {

constexpr int PS_TX = 32, PS_TY = 16, PS_THREADS = PS_TX * PS_TY;
constexpr int PS_MAX_S = 15, PS_MAX_P = 4, PS_MAX_K = 32;
constexpr int PS_TILE_FLOATS = (PS_TY + 2 * (PS_MAX_S + PS_MAX_P)) * (PS_TX + 2 * (PS_MAX_S + PS_MAX_P));
constexpr int PS_ROWF_FLOATS = (PS_TY + 2 * PS_MAX_P) * PS_TX;
constexpr unsigned PS_EMPTY = 0xffffffffu;

// exp(-x), x >= 0 (docs/kernels/nltv.md): y = min(x log2(e), 126), n = rint(y), a degree-7 polynomial of exp(-r ln 2) in
// r = y - n by Horner with every product and sum rounded, scaled by 2^-n
__host__ __device__ __forceinline__ float wexp(float x)
{
    const float y = fminf(x * (float)1.4426950408889634, 126.0f);
    const float n = rintf(y);
    const float r = y - n;
    float p = (float)-1.5252733804059840e-05;
    p = p * r; p = p + (float)0.0001540353039338161;
    p = p * r; p = p + (float)-0.0013333558146428443;
    p = p * r; p = p + (float)0.009618129107628477;
    p = p * r; p = p + (float)-0.05550410866482158;
    p = p * r; p = p + (float)0.2402265069591007;
    p = p * r; p = p + (float)-0.6931471805599453;
    p = p * r; p = p + (float)1.0;
    return ldexpf(p, -(int)n);
}

struct PatchArgs {
    const float *a;        // [nz][ny][nx]
    unsigned short *hi;    // [K][nz][ny][nx]
    unsigned short *hj;
    float *w;
    int nx, ny;
    size_t nvox;           // nz * ny * nx of the whole call: the stride between the tables' neighbour planes
    int S, K;
    float inv;             // 1 / h^2
    float g[2 * PS_MAX_P + 1];
};

template <int P, int KB>
__global__ __launch_bounds__(PS_THREADS) void patch_select_kernel(const PatchArgs q)
{
    __shared__ float tile[PS_TILE_FLOATS];
    __shared__ float rowf[2][PS_ROWF_FLOATS];

    const int tid = threadIdx.x;
    const int tx = tid % PS_TX, ty = tid / PS_TX;
    const int x0 = blockIdx.x * PS_TX, y0 = blockIdx.y * PS_TY;
    const int nx = q.nx, ny = q.ny, S = q.S;
    const int R = S + P;                       // the apron
    const int W = PS_TX + 2 * R, H = PS_TY + 2 * R;
    const size_t slice = (size_t)blockIdx.z * ((size_t)nx * ny);
    const float *a = q.a + slice;

    // the tile with its apron; pixels outside the slice are 0 and never contribute (their terms are masked below)
    for (int e = tid; e < W * H; e += PS_THREADS) {
        const int r = e / W, c = e - r * W;
        const int y = y0 - R + r, x = x0 - R + c;
        tile[e] = (y >= 0 && y < ny && x >= 0 && x < nx) ? a[(size_t)y * nx + x] : 0.0f;
    }
    __syncthreads();

    unsigned key[KB];
    int id[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) { key[s] = PS_EMPTY; id[s] = 0; }

    const int x = x0 + tx, y = y0 + ty;
    const int side = 2 * S + 1;
    int parity = 0;
    for (int jm = -S; jm <= S; ++jm) {
        // no pixel of the tile has a neighbour in this row of offsets (uniform over the workgroup)
        if (y0 + jm > ny - 1 || y0 + PS_TY - 1 + jm < 0) continue;
        for (int im = -S; im <= S; ++im) {
            if (jm == 0 && im == 0) continue;
            if (x0 + im > nx - 1 || x0 + PS_TX - 1 + im < 0) continue;
            float *rf = rowf[parity];
            parity ^= 1;
            // rowf(yr, xc) = sum_t g[t] D(yr, xc + t - P) for the rows the tile's column filters read
            for (int e = tid; e < (PS_TY + 2 * P) * PS_TX; e += PS_THREADS) {
                const int ry = e / PS_TX, cx = e - ry * PS_TX;
                const int yr = y0 - P + ry, xc = x0 + cx;
                float acc = 0.0f;
                if (yr >= 0 && yr < ny && yr + jm >= 0 && yr + jm < ny) {
                    const float *pa = tile + (ry + S) * W + (cx + S);
                    const float *pb = pa + jm * W + im;
#pragma unroll
                    for (int t = 0; t <= 2 * P; ++t) {
                        const int xx = xc + t - P;
                        const bool ok = xx >= 0 && xx < nx && xx + im >= 0 && xx + im < nx;
                        const float df = pa[t] - pb[t];
                        const float D = ok ? df * df : 0.0f;
                        acc = acc + q.g[t] * D;
                    }
                }
                rf[e] = acc;
            }
            __syncthreads();
            // d(y, x) = sum_t g[t] rowf(y + t - P, x), inserted where the candidate lies inside the slice
            const bool valid = x < nx && y < ny && x + im >= 0 && x + im < nx && y + jm >= 0 && y + jm < ny;
            float d = 0.0f;
#pragma unroll
            for (int t = 0; t <= 2 * P; ++t) d = d + q.g[t] * rf[(ty + t) * PS_TX + tx];
            const unsigned kd = __builtin_bit_cast(unsigned, d);
            if (valid && kd < key[KB - 1]) {
                unsigned ck = kd;
                int ci = (jm + S) * side + (im + S);
#pragma unroll
                for (int s = 0; s < KB; ++s) {
                    const bool lt = kd < key[s];   // once true, true for every later slot: the rest of the list shifts
                    const unsigned ok_ = key[s];
                    const int oi = id[s];
                    key[s] = lt ? ck : ok_;
                    id[s] = lt ? ci : oi;
                    ck = lt ? ok_ : ck;
                    ci = lt ? oi : ci;
                }
            }
        }
    }

    if (x >= nx || y >= ny) return;
    const size_t at = slice + (size_t)y * nx + x;
#pragma unroll
    for (int s = 0; s < KB; ++s) {
        if (s >= q.K) continue;
        const bool filled = key[s] != PS_EMPTY;
        const int mj = id[s] / side, mi = id[s] - mj * side;
        const size_t o = (size_t)s * q.nvox + at;
        q.hi[o] = (unsigned short)(filled ? x + mi - S : x);
        q.hj[o] = (unsigned short)(filled ? y + mj - S : y);
        q.w[o] = filled ? wexp(__builtin_bit_cast(float, key[s]) * q.inv) : 0.0f;
    }
}

struct NltvArgs {
    const float *f, *u_in;
    float *u_out;
    const unsigned short *hi, *hj;
    const float *w;
    int nx, ny, K;
    size_t nvox;
    float mu;   // 1 / lambda
};

__global__ __launch_bounds__(256) void nltv_iter_kernel(const NltvArgs q)
{
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= q.nvox) return;
    const size_t plane = (size_t)q.nx * q.ny;
    const size_t in_slice = at % plane;
    const float *us = q.u_in + (at - in_slice);   // the pixel's slice
    const float u = q.u_in[at];
    float s = 0.0f, val = 0.0f, nw = 0.0f;
    // unrolled so that the table loads, then the gathers, of eight neighbours are in flight together: one neighbour at a
    // time leaves the launch waiting on memory latency (docs/kernels/nltv.md, "Speed")
#pragma unroll 8
    for (int k = 0; k < q.K; ++k) {
        const size_t o = (size_t)k * q.nvox + at;
        const int i = min((int)q.hi[o], q.nx - 1), j = min((int)q.hj[o], q.ny - 1);
        const float wk = q.w[o];
        const float uk = us[(size_t)j * q.nx + i];
        const float df = uk - u;
        s = s + wk * (df * df);
        val = val + wk * uk;
        nw = nw + wk;
    }
    const float c = 2.0f / sqrtf(s + 1e-12f);
    q.u_out[at] = (q.mu * q.f[at] + c * val) / (q.mu + c * nw);
}

template <int P>
static void patch_select_launch(const PatchArgs &q, int kb, dim3 grid, hipStream_t st)
{
    if (kb == 8) patch_select_kernel<P, 8><<<grid, PS_THREADS, 0, st>>>(q);
    else if (kb == 16) patch_select_kernel<P, 16><<<grid, PS_THREADS, 0, st>>>(q);
    else patch_select_kernel<P, 32><<<grid, PS_THREADS, 0, st>>>(q);
}

static int nltv_dims_check(const char *op, int device, int dx, int dy, int dz, int nd)
{
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");
    TOMO_REQUIRE(nd == 2 || nd == 3, "2D or 3D arrays must be provided only");
    TOMO_REQUIRE(dx >= 1 && dy >= 1 && (nd == 2 || dz >= 1), "%s needs every dimension >= 1", op);
    TOMO_REQUIRE(dx <= 65535 && dy <= 65535, "%s: a slice of %d x %d exceeds the 65535 a 16-bit index table addresses", op, dx, dy);
    return TOMO_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_nltv_scratch_bytes(int dx, int dy, int dz, int nd) { return march_scratch_bytes(dx, dy, dz, nd); }

extern "C" int tomo_patch_select(int device, const float *in_dev, uint16_t *hi_dev, uint16_t *hj_dev, float *w_dev,
                                 int dx, int dy, int dz, int nd, int search, int patch, int neighbours, float h, void *stream)
{
    if (int rc = nltv_dims_check("PatchSelect", device, dx, dy, dz, nd)) return rc;
    if (nd == 2) dz = 1;
    TOMO_REQUIRE(search >= 1 && search <= PS_MAX_S, "PatchSelect: the search window must lie in [1, %d]", PS_MAX_S);
    TOMO_REQUIRE(patch >= 1 && patch <= PS_MAX_P, "PatchSelect: the patch window must lie in [1, %d]", PS_MAX_P);
    TOMO_REQUIRE(neighbours >= 1 && neighbours <= PS_MAX_K, "PatchSelect: the number of neighbours must lie in [1, %d]", PS_MAX_K);
    TOMO_REQUIRE(h > 0.0f, "PatchSelect: the edge parameter h must be positive");
    TOMO_REQUIRE(in_dev && hi_dev && hj_dev && w_dev, "NULL data pointer");
    TOMO_ON_DEVICE(device);
    hipStream_t st = as_stream(stream);

    PatchArgs q{};
    q.nx = dx; q.ny = dy;
    q.nvox = (size_t)dx * dy * dz;
    q.S = search; q.K = neighbours;
    q.inv = 1.0f / (h * h);
    for (int t = 0; t <= 2 * patch; ++t) {
        const int k = t - patch;
        q.g[t] = wexp((float)(k * k) / (float)(2 * patch * patch));
    }
    const int kb = neighbours <= 8 ? 8 : neighbours <= 16 ? 16 : 32;
    const size_t plane = (size_t)dx * dy;
    constexpr int max_z = 65535;   // slices per launch: the limit of grid z
    for (int z0 = 0; z0 < dz; z0 += max_z) {
        q.a = in_dev + (size_t)z0 * plane;
        q.hi = hi_dev + (size_t)z0 * plane;
        q.hj = hj_dev + (size_t)z0 * plane;
        q.w = w_dev + (size_t)z0 * plane;
        const dim3 grid(ceil_div(dx, PS_TX), ceil_div(dy, PS_TY), dz - z0 < max_z ? dz - z0 : max_z);
        switch (patch) {
        case 1: patch_select_launch<1>(q, kb, grid, st); break;
        case 2: patch_select_launch<2>(q, kb, grid, st); break;
        case 3: patch_select_launch<3>(q, kb, grid, st); break;
        default: patch_select_launch<4>(q, kb, grid, st); break;
        }
        TOMO_LAUNCH_CHECK();
    }
    return TOMO_OK;
}

extern "C" int tomo_nltv(int device, const float *in_dev, float *out_dev, const uint16_t *hi_dev, const uint16_t *hj_dev,
                         const float *w_dev, int dx, int dy, int dz, int nd, int neighbours, float lambda, int iters,
                         double tol, int *iters_done, double *last_rel_change, void *stream)
{
    if (int rc = nltv_dims_check("NLTV", device, dx, dy, dz, nd)) return rc;
    TOMO_REQUIRE(neighbours >= 1 && neighbours <= PS_MAX_K, "NLTV: the number of neighbours must lie in [1, %d]", PS_MAX_K);
    TOMO_REQUIRE(lambda > 0.0f, "NLTV: lambda must be positive");
    TOMO_REQUIRE(hi_dev && hj_dev && w_dev, "NULL table pointer");
    const size_t nvox = (size_t)dx * dy * (nd == 2 ? 1 : dz);
    TOMO_REQUIRE((nvox + 255) / 256 <= 0x7fffffffu, "volume too large for one NLTV launch");
    NltvArgs q{in_dev, nullptr, nullptr, hi_dev, hj_dev, w_dev, dx, dy, neighbours, nvox, 1.0f / lambda};
    return march_run("NLTV", device, in_dev, out_dev, dx, dy, dz, nd, iters, tol, iters_done, last_rel_change, stream,
                     [&](const float *u_in, float *u_out) {
                         q.u_in = u_in; q.u_out = u_out;
                         nltv_iter_kernel<<<(unsigned)((nvox + 255) / 256), 256, 0, as_stream(stream)>>>(q);
                         TOMO_LAUNCH_CHECK();
                         return (int)TOMO_OK;
                     });
}
