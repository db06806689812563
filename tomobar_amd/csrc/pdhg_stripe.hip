// The two launches PDHG's stripe variable adds (docs/kernels/pdhg.md, "The stripe variable"; include/tomo_mi355x.h):
//     min_{x, s} F(A x + S s; b) + lambda R(x) + mu |s|_1,     (S s)[z][a][u] = s[z][u],
// one offset per detector pixel, constant along the angles -- the ring artefact of a defective pixel, kept out of the image.
//   sino_dual_stripe_kernel   step 2 with e = r + s-bar in place of r, and in the same pass the sum of the new y along the
//                             angles of one segment of 64 rows: S^T y, which step 6 needs, without a second read of y
//   stripe_update_kernel      step 6: c = the sum of the segments' partial sums, s' = soft(s - tau_s c, theta), s-bar = 2 s' - s
// There is no reference implementation: tests/_pdhg_stripe_oracle.py restates both in numpy and the kernels reproduce its
// float32 form bit for bit (one rounding per operation in the stated order, no FMA contraction: -ffp-contract=off and no
// fmaf here; sqrtf and / are the compiler's correctly rounded ones).  The data terms are those of pdhg_kernels.hip: both
// read them from pdhg_data_term.h.
//
// Traffic of the fused launch: y read and written, r and b read (with a step per sample: sigma too) = 16 (20) B per sample,
// plus s-bar read and one partial sum written per (segment, z, u): (1 + 1) x 4 / 64 = 0.06 B per sample at full segments.
#include "tomo_common.h"
#include "pdhg_data_term.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>

namespace {

constexpr int SEG = TOMO_PDHG_STRIPE_SEG;   // rows of one segment: the chain of dependent adds of one partial sum
constexpr int SD_BLOCK = 64;                // one wave per workgroup: 4 columns per lane, 256 columns
constexpr int SD_COLS = 4;
constexpr int SD_ROWS = 4;                  // rows whose loads are issued before the first of them is used
constexpr int SD_MAX_GRID_YZ = 65535;       // planes and segments beyond it are walked by a stride loop
constexpr int UP_BLOCK = 256;

typedef float v4f __attribute__((ext_vector_type(4)));

// The SD_COLS values a lane owns of one row starting at `p`.  VEC: columns u[0] .. u[0] + 3, one 16-byte access; else the
// columns u[j] that lie inside the row (ok[j]), one 4-byte access each.  NT: the array is read once and not again soon.
template <bool VEC, bool NT>
__device__ __forceinline__ void row_load(float (&v)[SD_COLS], const float *p, const int (&u)[SD_COLS], const bool (&ok)[SD_COLS])
{
    if (VEC) {
        const v4f *q = reinterpret_cast<const v4f *>(p + u[0]);
        const v4f t = NT ? __builtin_nontemporal_load(q) : *q;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < SD_COLS; ++j) v[j] = ok[j] ? (NT ? __builtin_nontemporal_load(p + u[j]) : p[u[j]]) : 0.0f;
    }
}

template <bool VEC>
__device__ __forceinline__ void row_store(float *p, const float (&v)[SD_COLS], const int (&u)[SD_COLS], const bool (&ok)[SD_COLS])
{
    if (VEC) {
        *reinterpret_cast<v4f *>(p + u[0]) = v4f{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < SD_COLS; ++j)
            if (ok[j]) p[u[j]] = v[j];
    }
}

struct StripeDualArgs {
    float *y;             // [nz][na][nu], read and written
    const float *r, *b;   // like y, read once
    const float *sg;      // DIAG: the step per sample, like y
    const float *sbar;    // [nz][nu]
    float *part;          // [n_seg][nz][nu]
    int nz, na, nu, n_seg;
    float sigma, one_sigma, c4;
};

// Grid (u-blocks, z, segment).  A lane owns SD_COLS columns (VEC: consecutive ones; else lane + 64 j, so that the 4-byte
// accesses of a wave are consecutive) and marches the rows of its segment, nu apart, SD_ROWS at a time; s-bar is loaded
// once, y is updated in place and the lane's partial sums are written once.
template <int MODE, bool DIAG, bool VEC>
__global__ __launch_bounds__(SD_BLOCK) void sino_dual_stripe_kernel(StripeDualArgs a)
{
    const int base = (int)blockIdx.x * (SD_BLOCK * SD_COLS);
    int u[SD_COLS];
    bool ok[SD_COLS];
#pragma unroll
    for (int j = 0; j < SD_COLS; ++j) {
        u[j] = VEC ? base + (int)threadIdx.x * SD_COLS + j : base + (int)threadIdx.x + SD_BLOCK * j;
        ok[j] = u[j] < a.nu;
    }
    if (!ok[0]) return;   // u[0] is the lane's first column in both forms (VEC: nu % 4 == 0, so all four are inside)
    const size_t nu = (size_t)a.nu;

    auto one_row = [&](size_t off, const float (&sb)[SD_COLS], float (&acc)[SD_COLS], const float (&Y)[SD_COLS],
                       const float (&R)[SD_COLS], const float (&B)[SD_COLS], const float (&S)[SD_COLS]) __attribute__((always_inline)) {
        float out[SD_COLS];
#pragma unroll
        for (int j = 0; j < SD_COLS; ++j) {
            const float e = R[j] + sb[j];
            out[j] = DIAG ? data_prox<MODE>(Y[j], e, B[j], S[j], 1.0f + S[j], 4.0f * S[j])
                          : data_prox<MODE>(Y[j], e, B[j], a.sigma, a.one_sigma, a.c4);
            acc[j] = acc[j] + out[j];
        }
        row_store<VEC>(a.y + off, out, u, ok);
    };

    for (int z = (int)blockIdx.y; z < a.nz; z += (int)gridDim.y) {
        float sb[SD_COLS];
        row_load<VEC, false>(sb, a.sbar + (size_t)z * nu, u, ok);
        for (int k = (int)blockIdx.z; k < a.n_seg; k += (int)gridDim.z) {
            const int a0 = k * SEG;
            const int a1 = a.na - a0 < SEG ? a.na : a0 + SEG;
            float acc[SD_COLS];
#pragma unroll
            for (int j = 0; j < SD_COLS; ++j) acc[j] = 0.0f;
            int row = a0;
            for (; row + SD_ROWS <= a1; row += SD_ROWS) {
                float Y[SD_ROWS][SD_COLS], R[SD_ROWS][SD_COLS], B[SD_ROWS][SD_COLS], S[SD_ROWS][SD_COLS] = {};
#pragma unroll
                for (int i = 0; i < SD_ROWS; ++i) {
                    const size_t off = ((size_t)z * a.na + (row + i)) * nu;
                    row_load<VEC, false>(Y[i], a.y + off, u, ok);
                    row_load<VEC, true>(R[i], a.r + off, u, ok);
                    row_load<VEC, true>(B[i], a.b + off, u, ok);
                    if (DIAG) row_load<VEC, true>(S[i], a.sg + off, u, ok);
                }
#pragma unroll
                for (int i = 0; i < SD_ROWS; ++i) one_row(((size_t)z * a.na + (row + i)) * nu, sb, acc, Y[i], R[i], B[i], S[i]);
            }
            for (; row < a1; ++row) {
                const size_t off = ((size_t)z * a.na + row) * nu;
                float Y[SD_COLS], R[SD_COLS], B[SD_COLS], S[SD_COLS] = {};
                row_load<VEC, false>(Y, a.y + off, u, ok);
                row_load<VEC, true>(R, a.r + off, u, ok);
                row_load<VEC, true>(B, a.b + off, u, ok);
                if (DIAG) row_load<VEC, true>(S, a.sg + off, u, ok);
                one_row(off, sb, acc, Y, R, B, S);
            }
            row_store<VEC>(a.part + ((size_t)k * a.nz + z) * nu, acc, u, ok);
        }
    }
}

// the only launch site of the fused kernel
template <int MODE, bool DIAG>
static void stripe_dual_launch(const StripeDualArgs &a, bool vec, hipStream_t st)
{
    const int cols = SD_BLOCK * SD_COLS;
    const dim3 grid((unsigned)((a.nu + cols - 1) / cols), (unsigned)std::min(a.nz, SD_MAX_GRID_YZ),
                    (unsigned)std::min(a.n_seg, SD_MAX_GRID_YZ));
    if (vec)
        sino_dual_stripe_kernel<MODE, DIAG, true><<<grid, SD_BLOCK, 0, st>>>(a);
    else
        sino_dual_stripe_kernel<MODE, DIAG, false><<<grid, SD_BLOCK, 0, st>>>(a);
}

template <bool DIAG>
static void stripe_dual_run(int fidelity, const StripeDualArgs &a, bool vec, hipStream_t st)
{
    if (fidelity == TOMO_PDHG_LS) stripe_dual_launch<TOMO_PDHG_LS, DIAG>(a, vec, st);
    else if (fidelity == TOMO_PDHG_L1) stripe_dual_launch<TOMO_PDHG_L1, DIAG>(a, vec, st);
    else stripe_dual_launch<TOMO_PDHG_KL, DIAG>(a, vec, st);
}

// Step 6 over count = nz nu elements; part[k] starts k count floats in.  VEC: four elements per thread, 16-byte accesses
// (count % 4 == 0 and the three arrays 16-byte aligned); else one element per thread.
template <bool VEC>
__global__ __launch_bounds__(UP_BLOCK) void stripe_update_kernel(float *s, float *sbar, const float *part, size_t count, int n_seg,
                                                                float tau_s, float theta)
{
    constexpr int W = VEC ? 4 : 1;
    const size_t i = ((size_t)blockIdx.x * UP_BLOCK + threadIdx.x) * W;
    if (i >= count) return;
    float c[4] = {0.0f, 0.0f, 0.0f, 0.0f}, S[4] = {}, sn[4] = {}, sb[4] = {};   // W of the four are in use
    for (int k = 0; k < n_seg; ++k) {
        const float *p = part + (size_t)k * count + i;
        if (VEC) {
            const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p));
            c[0] = c[0] + t.x;
            c[1] = c[1] + t.y;
            c[2] = c[2] + t.z;
            c[3] = c[3] + t.w;
        } else {
            c[0] = c[0] + __builtin_nontemporal_load(p);
        }
    }
    if (VEC) {
        const v4f t = *reinterpret_cast<const v4f *>(s + i);
        S[0] = t.x; S[1] = t.y; S[2] = t.z; S[3] = t.w;
    } else {
        S[0] = s[i];
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const float w = S[j] - tau_s * c[j];
        sn[j] = w > theta ? w - theta : (w < -theta ? w + theta : 0.0f);
        sb[j] = (sn[j] + sn[j]) - S[j];
    }
    if (VEC) {
        *reinterpret_cast<v4f *>(s + i) = v4f{sn[0], sn[1], sn[2], sn[3]};
        *reinterpret_cast<v4f *>(sbar + i) = v4f{sb[0], sb[1], sb[2], sb[3]};
    } else {
        s[i] = sn[0];
        sbar[i] = sb[0];
    }
}

static bool aligned16(std::initializer_list<const void *> ptrs)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15u) == 0;
}

}  // namespace

extern "C" int tomo_pdhg_sino_dual_stripe(float *y_dev, const float *r_dev, const float *b_dev, const float *sigma_dev,
                                          const float *sbar_dev, float *part_dev, int nz, int na, int nu, int fidelity,
                                          float sigma, void *stream)
{
    TOMO_REQUIRE(known_fidelity(fidelity), "PDHG: the data term must be TOMO_PDHG_LS, TOMO_PDHG_L1 or TOMO_PDHG_KL");
    TOMO_REQUIRE(nz >= 1 && na >= 1 && nu >= 1, "PDHG: the stripe launches need nz, na and nu >= 1");
    TOMO_REQUIRE(sigma_dev || positive_finite(sigma), "PDHG: the step size sigma must be positive");
    TOMO_REQUIRE(y_dev && r_dev && b_dev && sbar_dev && part_dev, "NULL data pointer");
    for (const float *p : {r_dev, b_dev, sigma_dev, sbar_dev, static_cast<const float *>(part_dev)})
        TOMO_REQUIRE(p != y_dev, "PDHG: the dual array must not alias another array of the launch");
    for (const float *p : {r_dev, b_dev, sigma_dev, sbar_dev})
        TOMO_REQUIRE(p != part_dev, "PDHG: the partial sums must not alias another array of the launch");
    StripeDualArgs a{};
    a.y = y_dev; a.r = r_dev; a.b = b_dev; a.sg = sigma_dev; a.sbar = sbar_dev; a.part = part_dev;
    a.nz = nz; a.na = na; a.nu = nu; a.n_seg = (na + SEG - 1) / SEG;
    if (!sigma_dev) { a.sigma = sigma; a.one_sigma = 1.0f + sigma; a.c4 = 4.0f * sigma; }
    // a row starts nu floats after the one before: every access of the 16-byte form is aligned only if nu % 4 == 0 too
    const bool vec = nu % 4 == 0 && aligned16({y_dev, r_dev, b_dev, sigma_dev, sbar_dev, part_dev});
    if (sigma_dev) stripe_dual_run<true>(fidelity, a, vec, as_stream(stream));
    else stripe_dual_run<false>(fidelity, a, vec, as_stream(stream));
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

extern "C" int tomo_pdhg_stripe_update(float *s_dev, float *sbar_dev, const float *part_dev, int nz, int na, int nu, float tau_s,
                                       float theta, void *stream)
{
    TOMO_REQUIRE(nz >= 1 && na >= 1 && nu >= 1, "PDHG: the stripe launches need nz, na and nu >= 1");
    TOMO_REQUIRE(positive_finite(tau_s), "PDHG: the step size tau_s must be positive");
    TOMO_REQUIRE(theta >= 0.0f && std::isfinite(theta), "PDHG: the threshold theta = tau_s mu must be finite and not negative");
    TOMO_REQUIRE(s_dev && sbar_dev && part_dev, "NULL data pointer");
    TOMO_REQUIRE(s_dev != sbar_dev && part_dev != s_dev && part_dev != sbar_dev, "PDHG: s, s-bar and the partial sums must not alias");
    const size_t count = (size_t)nz * (size_t)nu;
    const int n_seg = (na + SEG - 1) / SEG;
    const bool vec = count % 4 == 0 && aligned16({s_dev, sbar_dev, part_dev});
    const size_t threads = vec ? count / 4 : count;
    const size_t grid = (threads + UP_BLOCK - 1) / UP_BLOCK;
    TOMO_REQUIRE(grid <= 0x7fffffffu, "PDHG: %zu stripe offsets exceed one launch", count);
    if (vec)
        stripe_update_kernel<true><<<(unsigned)grid, UP_BLOCK, 0, as_stream(stream)>>>(s_dev, sbar_dev, part_dev, count, n_seg, tau_s, theta);
    else
        stripe_update_kernel<false><<<(unsigned)grid, UP_BLOCK, 0, as_stream(stream)>>>(s_dev, sbar_dev, part_dev, count, n_seg, tau_s, theta);
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}
