// Parallel-beam 3D projector pair for gfx950 with the FISTA / ADMM epilogues fused in.
//
// Model (fixed by the reference's geometry, supp/funcs.py:45-65, and by the ASTRA operators it calls at
// astra_base.py:554,601; restated in oracle/tomo_oracle.c):
//   BP  voxel-driven: vol[z,y,x] = sum_a lerp_u( sino[z,a,:], x_w cos + y_w sin - cor + nu/2 - 1/2 )
//   FP  ray-driven Joseph: step along the dominant axis, 2-tap linear interpolation along the other in-plane
//       axis, zero outside the volume, scaled by the ray length per step.
// MI355X mapping:
//   * BP variant 0 ("brick", bp_brick.inl): a 256-thread workgroup owns a 32(x) x 16(y) x 16(z) voxel brick, a
//     wave a 16 x 4 patch of it.  For a batch of 8 angles the [angle][z-quad][u] window of the sinogram that the
//     brick can touch is staged in LDS as float4 over z: one ds_read_b128 per tap serves four slices,
//     interpolation index/weights are computed once per (voxel column, angle) and reused by all 16 slices.
//     Workgroups are numbered so that each XCD's L2 sees one z-batch of sinogram rows at a time.
//   * BP variant 2 ("tiled"): the first LDS kernel (64 x 8 x 16 brick, lanes along x), kept for A/B runs.
//   * BP variant 1 ("direct"): taps straight from global memory (L1/L2), 4 slices per thread.
//   * FP (fp_tiled.inl): one lane per detector pixel, 8 angles x 4 slices per lane, sequential march over the
//     volume rows staged in LDS (bit-identical to the oracle); x-stepping angles read an in-plane transposed
//     copy of the volume so that the interpolation axis is always the contiguous one.  Variant 1: no LDS.
//   * epilogues: plain / residual (FP) and plain / FISTA step / FISTA step+momentum / ADMM z-update (BP).
// No MFMA: there is no dense contraction on this path.
#include "bp_common.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------ shared pieces
// Robust re-weighting of a data residual (the Huber and Student's-t data terms of the reference's removed RecToolsIR class:
// _data_["huber_threshold"], _data_["studentst_threshold"], Demos/methods_IR_legacy/DemoFISTA_artifacts2D.py:197,348;
// formula-level, see include/tomo_mi355x.h): Huber  r <- (delta/|r|) r where |r| > delta;  Student's t  r <- (2/(delta^2 + r^2)) r
__device__ __forceinline__ float robust_weight(float r, int mode, float delta)
{
    if (mode == TOMO_ROBUST_HUBER) {
        const float ar = fabsf(r);
        if (ar > delta) r = (delta / ar) * r;
    } else if (mode == TOMO_ROBUST_STUDENTST) {
        r = (2.0f / (delta * delta + r * r)) * r;
    }
    return r;
}

// The epilogues of the voxel-driven kernels: the loads and stores around bp_value (bp_common.h), which holds the arithmetic.
template <int EPI>
__device__ __forceinline__ void bp_epilogue(const BpArgs &a, size_t idx, float g)
{
    float o0 = 0.0f, o1 = 0.0f;
    if (EPI == EPI_PLAIN) {
        a.vol[idx] = g;
    } else if (EPI == EPI_FISTA) {
        bp_value<EPI>(a, g, a.xt[idx], 0.0f, 0.0f, o0, o1);
        a.xout[idx] = o0;
    } else if (EPI == EPI_FISTA_MOM) {
        bp_value<EPI>(a, g, a.xt[idx], a.xold[idx], 0.0f, o0, o1);
        a.xout[idx] = o0;
        a.xt_out[idx] = o1;
    } else {
        bp_value<EPI>(a, g, a.xout[idx], a.xold[idx], a.xt[idx], o0, o1);
        a.xout[idx] = o0;
        a.xt_out[idx] = o1;
    }
}

// the same epilogues on four consecutive voxels of a row (idx a multiple of 4, 16-byte aligned arrays): one dwordx4 access
// per array instead of four dword accesses
template <int EPI>
__device__ __forceinline__ void bp_epilogue4(const BpArgs &a, size_t idx, float4 g4)
{
    // The epilogue's volume streams are touched once (X_t read, X written: 8.6 GB through a 4 MB L2 per 1024^3 call) while the
    // sinogram windows of a z-brick (4.9 MB) are re-read by every brick of the XCD: with ordinary loads / stores the streams
    // evict the windows and the L2 re-fetches them ~33 x from the fabric (14.6 GB per call); marked NON-TEMPORAL they leave the
    // windows resident -- fetch 14.6 -> 4.9 GB (X_t + 1.8 x the subset), call 7.09 -> 6.90 ms (profiles/r5i_bp_epilogue_nontemporal_ab.txt).
    auto ld4 = [&](const float *p) { return __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p + idx)); };
    auto st4 = [&](float *p, v4f v) { __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(p + idx)); };
    const v4f g = v4f{g4.x, g4.y, g4.z, g4.w}, zero = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    if (EPI == EPI_PLAIN) {
        st4(a.vol, g);
        return;
    }
    v4f i0 = zero, i1 = zero, i2 = zero, o0 = zero, o1 = zero;
    if (EPI == EPI_FISTA) {
        i0 = ld4(a.xt);
    } else if (EPI == EPI_FISTA_MOM) {
        i0 = ld4(a.xt); i1 = ld4(a.xold);
    } else {
        i0 = ld4(a.xout); i1 = ld4(a.xold); i2 = ld4(a.xt);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float p = 0.0f, r = 0.0f;
        bp_value<EPI>(a, g[k], i0[k], i1[k], i2[k], p, r);
        o0[k] = p; o1[k] = r;
    }
    st4(a.xout, o0);
    if (EPI != EPI_FISTA) st4(a.xt_out, o1);
}

// ------------------------------------------------------------------------------------------ BP variant 1
template <int EPI, bool LERP8>
__global__ __launch_bounds__(256) void bp_direct_kernel(BpArgs a)
{
    constexpr int ZB = 4;
    const int ix = blockIdx.x * 64 + (threadIdx.x & 63);
    const int iy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int z0 = blockIdx.z * ZB;
    if (ix >= a.n || iy >= a.n) return;
    const float half_n = 0.5f * (float)a.n - 0.5f, half_u = 0.5f * (float)a.nu - 0.5f;
    const float xw = (float)ix - half_n, yw = (float)iy - half_n;
    float acc[ZB] = {0.0f, 0.0f, 0.0f, 0.0f};
    const size_t zstride = (size_t)a.na * a.nu;
    for (int k = 0; k < a.na; ++k) {
        const tomo_angle_t t = a.tab[k];
        const float off = half_u - t.cor;
        const float f = fmaf(xw, t.cs, fmaf(yw, t.sn, off));
        const float fl = floorf(f);
        const float w = lerp_w<LERP8>(f, fl), omw = 1.0f - w;
        const int i0 = (int)fl;
        const bool ok0 = (i0 >= 0) && (i0 < a.nu), ok1 = (i0 + 1 >= 0) && (i0 + 1 < a.nu);
        if (a.zquad) {  // uniform: the private residual layout, four slices per 16-byte word
            const float4 *row4 = reinterpret_cast<const float4 *>(a.sino) + ((size_t)(z0 >> 2) * a.na + k) * a.nu;
            const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float4 q0 = ok0 ? row4[i0] : zero4, q1 = ok1 ? row4[i0 + 1] : zero4;
            const float t0[ZB] = {q0.x, q0.y, q0.z, q0.w}, t1[ZB] = {q1.x, q1.y, q1.z, q1.w};
#pragma unroll
            for (int zz = 0; zz < ZB; ++zz) {
                acc[zz] = fmaf(omw, t0[zz], acc[zz]);
                acc[zz] = fmaf(w, t1[zz], acc[zz]);
            }
            continue;
        }
        const float *row = a.sino + ((size_t)z0 * a.na + k) * a.nu;
#pragma unroll
        for (int zz = 0; zz < ZB; ++zz) {
            const bool zok = z0 + zz < a.nz;
            const float s0 = (ok0 && zok) ? row[zz * zstride + i0] : 0.0f;
            const float s1 = (ok1 && zok) ? row[zz * zstride + i0 + 1] : 0.0f;
            acc[zz] = fmaf(omw, s0, acc[zz]);
            acc[zz] = fmaf(w, s1, acc[zz]);
        }
    }
#pragma unroll
    for (int zz = 0; zz < ZB; ++zz)
        if (z0 + zz < a.nz) bp_epilogue<EPI>(a, ((size_t)(z0 + zz) * a.n + iy) * a.n + ix, acc[zz]);
}

// ------------------------------------------------------------------------------------------ BP variant 0
constexpr int BP_TX = 64, BP_TY = 8, BP_RY = 2, BP_ZQ = 4, BP_AB = 8, BP_PITCH = 72;

template <int EPI, bool LERP8>
__global__ __launch_bounds__(256) void bp_tiled_kernel(BpArgs a)
{
    __shared__ float4 tile[BP_AB][BP_ZQ][BP_PITCH];  // 36 KiB
    __shared__ int umin_s[BP_AB];

    // XCD-aware numbering: workgroup b lands on XCD b%8; give each XCD its own z-batch stream
    const int ntiles = a.ntx * a.nty;
    const int b = blockIdx.x, xcd = b & 7, q = b >> 3;
    const int per_xcd = (a.nzb * ntiles + 7) >> 3;  // a contiguous eighth of the (z-batch, tile) list per XCD
    const int wi = xcd * per_xcd + q;
    if (wi >= a.nzb * ntiles) return;  // uniform for the workgroup
    const int zb = wi / ntiles;
    const int tid = wi % ntiles;
    const int tx0 = (tid % a.ntx) * BP_TX, ty0 = (tid / a.ntx) * BP_TY;
    const int z0 = zb * (4 * BP_ZQ);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ix = tx0 + lane;
    const float half_n = 0.5f * (float)a.n - 0.5f, half_u = 0.5f * (float)a.nu - 0.5f;
    const float xw = (float)ix - half_n;
    float yw[BP_RY];
#pragma unroll
    for (int r = 0; r < BP_RY; ++r) yw[r] = (float)(ty0 + wave * BP_RY + r) - half_n;

    float acc[BP_RY][4 * BP_ZQ];
#pragma unroll
    for (int r = 0; r < BP_RY; ++r)
#pragma unroll
        for (int j = 0; j < 4 * BP_ZQ; ++j) acc[r][j] = 0.0f;

    const size_t zstride = (size_t)a.na * a.nu;
    for (int a0 = 0; a0 < a.na; a0 += BP_AB) {
        const int nb = min(BP_AB, a.na - a0);
        __syncthreads();  // previous batch fully consumed
        if ((int)threadIdx.x < nb) {
            // detector window of the brick: the coordinate is monotone in x and in y, so the four corners bound it
            const tomo_angle_t t = a.tab[a0 + threadIdx.x];
            const float off = half_u - t.cor;
            const float x0 = (float)tx0 - half_n, x1 = (float)(tx0 + BP_TX - 1) - half_n;
            const float y0 = (float)ty0 - half_n, y1 = (float)(ty0 + BP_TY - 1) - half_n;
            const float f00 = fmaf(x0, t.cs, fmaf(y0, t.sn, off)), f10 = fmaf(x1, t.cs, fmaf(y0, t.sn, off));
            const float f01 = fmaf(x0, t.cs, fmaf(y1, t.sn, off)), f11 = fmaf(x1, t.cs, fmaf(y1, t.sn, off));
            umin_s[threadIdx.x] = (int)floorf(fminf(fminf(f00, f10), fminf(f01, f11)));
        }
        __syncthreads();
        // stage [angle][z-quad][u] as float4 over z: four coalesced row reads, one 16-byte LDS write
        for (int item = threadIdx.x; item < nb * BP_ZQ * BP_PITCH; item += 256) {
            const int j = item % BP_PITCH;
            const int zq = (item / BP_PITCH) % BP_ZQ;
            const int aa = item / (BP_PITCH * BP_ZQ);
            const int u = umin_s[aa] + j;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (u >= 0 && u < a.nu) {
                const int z = z0 + zq * 4;
                const float *p = a.sino + ((size_t)z * a.na + (a0 + aa)) * a.nu + u;
                if (z + 0 < a.nz) v.x = p[0];
                if (z + 1 < a.nz) v.y = p[zstride];
                if (z + 2 < a.nz) v.z = p[2 * zstride];
                if (z + 3 < a.nz) v.w = p[3 * zstride];
            }
            tile[aa][zq][j] = v;
        }
        __syncthreads();
        for (int aa = 0; aa < nb; ++aa) {
            const tomo_angle_t t = a.tab[a0 + aa];
            const float off = half_u - t.cor;
            const int um = umin_s[aa];
#pragma unroll
            for (int r = 0; r < BP_RY; ++r) {
                const float f = fmaf(xw, t.cs, fmaf(yw[r], t.sn, off));
                const float fl = floorf(f);
                const float w = lerp_w<LERP8>(f, fl), omw = 1.0f - w;
                const int idx = (int)fl - um;
#pragma unroll
                for (int zq = 0; zq < BP_ZQ; ++zq) {
                    const float4 s0 = tile[aa][zq][idx];
                    const float4 s1 = tile[aa][zq][idx + 1];
                    float *c = &acc[r][zq * 4];
                    c[0] = fmaf(omw, s0.x, c[0]); c[0] = fmaf(w, s1.x, c[0]);
                    c[1] = fmaf(omw, s0.y, c[1]); c[1] = fmaf(w, s1.y, c[1]);
                    c[2] = fmaf(omw, s0.z, c[2]); c[2] = fmaf(w, s1.z, c[2]);
                    c[3] = fmaf(omw, s0.w, c[3]); c[3] = fmaf(w, s1.w, c[3]);
                }
            }
        }
    }
    if (ix < a.n) {
#pragma unroll
        for (int r = 0; r < BP_RY; ++r) {
            const int iy = ty0 + wave * BP_RY + r;
            if (iy < a.n) {
#pragma unroll
                for (int j = 0; j < 4 * BP_ZQ; ++j)
                    if (z0 + j < a.nz) bp_epilogue<EPI>(a, ((size_t)(z0 + j) * a.n + iy) * a.n + ix, acc[r][j]);
            }
        }
    }
}

#include "bp_brick.inl"

// planar sinogram [nz][row] (row = na * nu) -> the quad-interleaved layout [ceil(nz/4)][row][4] the brick kernel stages by
// LDS-DMA; slices past nz are zeros.  One coalesced pass: 8 B per sample moved, ~0.13 ms for a 75-angle subset at 1024^3.
__global__ __launch_bounds__(256) void sino_to_quad_kernel(const float *__restrict__ in, float4 *__restrict__ out, int nz, size_t row)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int z = 4 * (int)blockIdx.y;
    if (i >= row) return;
    const float *p = in + (size_t)z * row + i;
    float4 v;
    v.x = p[0];
    v.y = z + 1 < nz ? p[row] : 0.0f;
    v.z = z + 2 < nz ? p[2 * row] : 0.0f;
    v.w = z + 3 < nz ? p[3 * row] : 0.0f;
    out[(size_t)blockIdx.y * row + i] = v;
}

constexpr size_t BP_RELAY_MAX_BYTES = (size_t)16 << 30;  // largest sinogram tomo_bp3d* re-lays into its scratch arena
// Smallest relay scratch a DEVICE could not provide (out of memory only): requests that large go straight to the planar staging
// instead of failing a hipMalloc per call.  Not for ever: another tenant's placement search or a framework's caching allocator
// may have held the memory for a moment, so every BP_RELAY_RETRY-th refused call asks again and tomo_release_scratch(device)
// forgets the refusal (tomo_bp_relay_reset).
constexpr int BP_RELAY_DEVICES = 64, BP_RELAY_RETRY = 64;
struct bp_relay_state { std::atomic<size_t> refused{~(size_t)0}; std::atomic<unsigned> skipped{0}; };
bp_relay_state g_bp_relay[BP_RELAY_DEVICES];

template <int EPI>
int bp_launch(BpArgs a, bool lerp8, hipStream_t st)
{
    TOMO_ON_DEVICE(a.device);
    tomo_prof_scope prof(PROF_BP, st, 1);
    a.epi_aligned = bp_epi_aligned<EPI>(a);
    // the brick kernel addresses a 16-slice sinogram slab with 32-bit element offsets
    // (the quad layout is read through one buffer descriptor per z-brick and batch: 4 quads x 16 bytes < 2^31)
    if (EPI == EPI_PLAIN) a.zquad = 0;  // tomo_bp3d always takes the public layout
    if (EPI != EPI_FISTA) a.xt_zquad = 0;
    if (a.xt_zquad) {  // only the brick kernel's epilogue reads the quad-interleaved X_t (tomo_ctx_volume_zquad_ok says so beforehand)
        TOMO_REQUIRE((((uintptr_t)a.xt) & 15) == 0, "the quad-interleaved volume must be 16-byte aligned");
        TOMO_REQUIRE((g_variant_bp == 0 || g_variant_bp == 3) && (long)a.na * a.nu < (1L << 25),
                     "this back projection does not read the quad-interleaved volume");
    }
    if (a.zquad && (((uintptr_t)a.sino) & 15) != 0)
        return tomo_fail(TOMO_E_INVALID, "the quad-interleaved residual must be 16-byte aligned");
    // A PLANAR sinogram (tomo_bp3d: FBP, SIRT, CGLS, OSEM, the power method; the fused epilogues of the ring-term and
    // vertical-CoR paths) is re-laid quad-interleaved into this stream's scratch arena first: one streaming pass (8 B per
    // sample) buys the LDS-DMA staging of the brick kernel -- 4 workgroups per CU, no staging registers -- which is worth 7 x
    // as much per 75-angle subset and 8 x for a whole angle set (docs/kernels/bp.md).  Not for sinograms beyond 16 GiB, not
    // when the arena cannot be had (then the planar staging runs), and not with bp variant 3 (dev flavour: planar staging, A/B).
    bool relaid = false;
    if (g_variant_bp == 0 && !a.zquad && (long)a.na * a.nu < (1L << 25) && a.na > 0) {
        const size_t row = (size_t)a.na * a.nu, nq = (size_t)ceil_div(a.nz, 4), bytes = nq * row * 16;
        void *q = nullptr;
        bp_relay_state &rs = g_bp_relay[a.device >= 0 && a.device < BP_RELAY_DEVICES ? a.device : 0];
        bool have = bytes <= BP_RELAY_MAX_BYTES && nq <= 65535;
        if (have && bytes >= rs.refused.load() && (rs.skipped.fetch_add(1) + 1) % BP_RELAY_RETRY != 0) have = false;
        if (have) {
            const int rc = tomo_arena_get(a.device, st, ARENA_BPQ, bytes, &q);
            if (rc == TOMO_E_NOMEM) {   // the planar staging runs, now and for the next requests this large on this device
                rs.refused.store(std::min(rs.refused.load(), bytes));
                tomo_warn_once("bp_relay", "back projection: no memory for the quad-interleaved relay of a planar sinogram, "
                                           "running the planar staging (slower; asked again every 64th call and after tomo_release_scratch)");
                have = false;
            } else if (rc != TOMO_OK) {
                return rc;   // a caller error or a runtime failure is reported, not papered over
            } else {
                rs.refused.store(~(size_t)0);
            }
        }
        if (have) {
            sino_to_quad_kernel<<<dim3((unsigned)((row + 255) / 256), (unsigned)nq), 256, 0, st>>>(a.sino, (float4 *)q, a.nz, row);
            TOMO_LAUNCH_CHECK();
            a.sino = (const float *)q;
            a.zquad = 1;
            relaid = true;
        }
    }
    const bool brick_ok = (long)a.na * a.nu < (a.zquad ? (1L << 25) : (1L << 27));
    const int variant = g_variant_bp == 3 ? 0 : g_variant_bp;  // 3 = the default kernel on the planar layout
    if (variant == 1 || (variant == 0 && !brick_ok)) {
        if (variant == 0)
            tomo_warn_once("bp_direct", "back projection: angles x detector >= 2^27 samples per slice, falling back to "
                                        "the direct (no LDS) kernel (about 3.5x slower)");
        if (a.path) *a.path = "direct(no LDS)";
        dim3 grid(ceil_div(a.n, 64), ceil_div(a.n, 4), ceil_div(a.nz, 4));
        if (lerp8) bp_direct_kernel<EPI, true><<<grid, 256, 0, st>>>(a);
        else bp_direct_kernel<EPI, false><<<grid, 256, 0, st>>>(a);
    } else if (variant == 0) {
        if (a.path) *a.path = "brick(32x16x16)";
        a.ntx = ceil_div(a.n, BB_TX);
        a.nty = ceil_div(a.n, BB_TY);
        a.nzb = ceil_div(a.nz, 4 * BB_ZQ);
        const long blocks = 8L * (((long)a.nzb * a.ntx * a.nty + 7) / 8);
        if (blocks > 0x7fffffffL) return tomo_fail(TOMO_E_INVALID, "volume too large for one BP launch");
        if (a.zquad) {
            if (a.path) *a.path = relaid ? "brick(32x16x16, planar sinogram re-laid quad-interleaved, LDS-DMA staging)"
                                         : "brick(32x16x16, quad-interleaved residual, LDS-DMA staging)";
            if (lerp8) bp_brick_kernel<EPI, true, true><<<(unsigned)blocks, 256, 0, st>>>(a);
            else bp_brick_kernel<EPI, false, true><<<(unsigned)blocks, 256, 0, st>>>(a);
            TOMO_LAUNCH_CHECK();
            return TOMO_OK;
        }
        if (lerp8) bp_brick_kernel<EPI, true><<<(unsigned)blocks, 256, 0, st>>>(a);
        else bp_brick_kernel<EPI, false><<<(unsigned)blocks, 256, 0, st>>>(a);
    }
#if TOMO_DEV
    else {  // variant 2 (dev flavour): the round-1 tiling with lanes along x, kept for A/B measurement
        if (a.zquad) return tomo_fail(TOMO_E_INVALID, "bp variant 2 reads the planar residual layout only");
        if (a.path) *a.path = "tiled(64x8x16)";
        a.ntx = ceil_div(a.n, BP_TX);
        a.nty = ceil_div(a.n, BP_TY);
        a.nzb = ceil_div(a.nz, 4 * BP_ZQ);
        const long blocks = 8L * (((long)a.nzb * a.ntx * a.nty + 7) / 8);
        if (blocks > 0x7fffffffL) return tomo_fail(TOMO_E_INVALID, "volume too large for one BP launch");
        if (lerp8) bp_tiled_kernel<EPI, true><<<(unsigned)blocks, 256, 0, st>>>(a);
        else bp_tiled_kernel<EPI, false><<<(unsigned)blocks, 256, 0, st>>>(a);
    }
#endif
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

// ------------------------------------------------------------------------------------------ FP
struct FpArgs {
    const float *vol;        // [nz][n][n]   (y rows, x contiguous)
    const float *volT;       // [nz][n][n]   (x rows, y contiguous) -- may be null when no angle steps along x
    const tomo_angle_t *tab;
    int nz, n, nu, na, na_full;
    float *out;              // [nz][na][nu]
    const float *b;          // residual epilogue: full sinogram [nz][na_full][nu] (null = plain FP)
    const float *w;          // PWLS weights, full sinogram (may be null)
    const float *ring;       // Group-Huber offsets [nz][nu] (may be null)
    float ring_scale;
    int fidelity;
    int gathered;            // bit0: b is the gathered subset, bit1: w is
    int zquad;               // residual epilogue: out is [ceil(nz/4)][na][nu][4] (TOMO_RESIDUAL_ZQUAD)
    int robust;              // TOMO_ROBUST_*: re-weighting of the LS / PWLS residual (Huber, Student's t)
    float rdelta;            // its threshold
};

// The residual epilogue of every forward-projection kernel (data_fidelities.py:28-39 + the ring offsets + the robust
// re-weightings): `val` = (A_s x)[z, k_a, iu]; Args = FpArgs or FpTiledArgs (same field names).
template <class Args>
__device__ __forceinline__ float fp_residual_value(const Args &a, float val, int z, int k_a, int src, int iu)
{
    const size_t gi = ((size_t)z * a.na + k_a) * a.nu + iu;          // gathered layout
    const size_t fi = ((size_t)z * a.na_full + src) * a.nu + iu;     // full-sinogram layout
    const float bv = a.b[(a.gathered & TOMO_GATHERED_B) ? gi : fi];
    if (a.fidelity == TOMO_FID_KL || a.fidelity == TOMO_FID_RATIO) {
        const float ax = val < 1e-8f ? 1e-8f : val;
        const float q = bv / ax;
        return (a.fidelity == TOMO_FID_KL) ? 1.0f - q : q;
    }
    val = val - bv;
    if (a.ring) val = val + a.ring_scale * a.ring[(size_t)z * a.nu + iu];
    if (a.w) val = val * a.w[(a.gathered & TOMO_GATHERED_W) ? gi : fi];
    return robust_weight(val, a.robust, a.rdelta);
}

// X_t = X + beta (X - X_old) (the momentum step of methodsIR_CuPy.py:475: mul then add, no fma) written twice: as is,
// and in-plane transposed into the forward projector's scratch copy -- the next forward projection of X_t then needs no
// transpose pass of its own (one read of X_t saved per sub-iteration).  MOMENTUM = false: the plain in-plane transpose of x
// into xt_T (xold, xt and beta unused).
template <bool MOMENTUM>
__global__ __launch_bounds__(256) void momentum_transpose_kernel(const float *__restrict__ x, const float *__restrict__ xold,
                                                                float *__restrict__ xt, float *__restrict__ xt_T, float beta, int n)
{
    __shared__ float t[32][33];
    const size_t zoff = (size_t)blockIdx.z * n * n;
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;  // 32 x 8
    for (int r = ly; r < 32; r += 8) {
        const int xx = bx + lx, yy = by + r;
        float v = 0.0f;
        if (xx < n && yy < n) {
            const size_t i = zoff + (size_t)yy * n + xx;
            v = x[i];
            if (MOMENTUM) {
                v = v + beta * (v - xold[i]);
                xt[i] = v;
            }
        }
        t[r][lx] = v;
    }
    __syncthreads();
    for (int r = ly; r < 32; r += 8) {
        const int yy = by + lx, xx = bx + r;
        if (xx < n && yy < n) xt_T[zoff + (size_t)xx * n + yy] = t[lx][r];
    }
}

// The same kernel on 64 x 64 tiles with 16-byte accesses (round 5): a wave reads four whole 256-byte row segments per
// instruction instead of two 128-byte ones, and the transposed tile leaves as float4 along y.  Needs n % 4 == 0 and 16-byte
// aligned arrays (the launchers fall back to the 32 x 32 dword kernels otherwise).  MOMENTUM = false: plain in-plane transpose.
// LDS tile [64][65]: the transposed read of lane (c, r) touches bank (4c + j + r) mod 64 -- conflict-free for every j.
// Every stream is touched once per call and is far larger than the L2: non-temporal accesses.  Same-box A/B at 1024^3 (momentum
// + transposed copy, profiles/r5w_momentum_tile_ab.txt): 32 x 32 dword 3.48 ms, 64 x 64 float4 3.34, + non-temporal 3.25.
typedef float glue_v4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_ld4(const float *p)
{
    const glue_v4 v = __builtin_nontemporal_load(reinterpret_cast<const glue_v4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_st4(float *p, float4 v)
{
    __builtin_nontemporal_store(glue_v4{v.x, v.y, v.z, v.w}, reinterpret_cast<glue_v4 *>(p));
}
template <bool MOMENTUM>
__global__ __launch_bounds__(256) void transpose64_kernel(const float *__restrict__ x, const float *__restrict__ xold,
                                                          float *__restrict__ xt, float *__restrict__ xt_T, float beta, int n)
{
    __shared__ float t[64][65];
    const size_t zoff = (size_t)blockIdx.z * n * n;
    const int bx = blockIdx.x * 64, by = blockIdx.y * 64;
    const int c4 = (threadIdx.x & 15) * 4, r0 = threadIdx.x >> 4;  // 16 float4 columns x 16 rows per pass
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + 16 * k;
        const int xx = bx + c4, yy = by + r;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (xx < n && yy < n) {
            const size_t i = zoff + (size_t)yy * n + xx;
            const float4 a = nt_ld4(x + i);
            if (MOMENTUM) {
                const float4 o = nt_ld4(xold + i);
                v.x = a.x + beta * (a.x - o.x); v.y = a.y + beta * (a.y - o.y);
                v.z = a.z + beta * (a.z - o.z); v.w = a.w + beta * (a.w - o.w);
                nt_st4(xt + i, v);
            } else {
                v = a;
            }
        }
        t[r][c4] = v.x; t[r][c4 + 1] = v.y; t[r][c4 + 2] = v.z; t[r][c4 + 3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + 16 * k;           // column of the tile = row of the transposed copy
        const int xx = bx + r, yy = by + c4;
        if (xx < n && yy < n)
            nt_st4(xt_T + zoff + (size_t)xx * n + yy, make_float4(t[c4][r], t[c4 + 1][r], t[c4 + 2][r], t[c4 + 3][r]));
    }
}

// The producers of the private volume layout TOMO_VOLUME_ZQUAD (round 7; tomo_mi355x.h): X_t = X + beta (X - X_old) (MOMENTUM;
// the same mul-then-add) or X_t = X, written QUAD-INTERLEAVED twice -- xq [nz/4][y][x][4] and, in-plane transposed,
// xq_T [nz/4][x][y][4] -- for the forward projector's LDS-DMA staging and the back projector's gradient-step epilogue.  No
// planar X_t exists, so this moves what transpose64_kernel<true> moves: two reads, two writes per voxel.  One workgroup
// takes a 64 x 64 tile of the FOUR slices of a quad, so every store is a whole float4; the padding slices of the last quad
// are written as zeros.  LDS tile [4][64][64] floats (the 64 KiB a static array may have), column rotated by the row: the
// planar float4 writes, the row-wise reads (bank = lane + row) and the transposed reads (bank = lane + column) are all
// conflict-free.  Needs n % 4 == 0 and 16-byte aligned arrays.
template <bool MOMENTUM>
__global__ __launch_bounds__(256) void zquad64_kernel(const float *__restrict__ x, const float *__restrict__ xold,
                                                      float *__restrict__ xq, float *__restrict__ xq_T, float beta, int n, int nz)
{
    __shared__ float t[4][64][64];
    const size_t plane = (size_t)n * n;
    const int z0 = 4 * (int)blockIdx.z;
    const int bx = blockIdx.x * 64, by = blockIdx.y * 64;
    const int c4 = (threadIdx.x & 15) * 4, r0 = threadIdx.x >> 4;  // 16 float4 columns x 16 rows per pass
    // all 16 (32 with X_old) loads of the thread are issued before the first value is used: two workgroups share a CU (LDS), so
    // the bytes in flight have to come from each wave
    float4 av[4][4], ov[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int zz = 0; zz < 4; ++zz) {
            const int xx = bx + c4, yy = by + r0 + 16 * k;
            av[k][zz] = ov[k][zz] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (xx < n && yy < n && z0 + zz < nz) {
                const size_t i = (size_t)(z0 + zz) * plane + (size_t)yy * n + xx;
                av[k][zz] = nt_ld4(x + i);
                if (MOMENTUM) ov[k][zz] = nt_ld4(xold + i);
            }
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + 16 * k;
#pragma unroll
        for (int zz = 0; zz < 4; ++zz) {
            const float4 a = av[k][zz], o = ov[k][zz];
            float4 v = a;   // (outside the volume a = o = 0 and the momentum of zeros is +0)
            if (MOMENTUM) {
                v.x = a.x + beta * (a.x - o.x); v.y = a.y + beta * (a.y - o.y);
                v.z = a.z + beta * (a.z - o.z); v.w = a.w + beta * (a.w - o.w);
            }
            t[zz][r][(c4 + r) & 63] = v.x; t[zz][r][(c4 + 1 + r) & 63] = v.y;
            t[zz][r][(c4 + 2 + r) & 63] = v.z; t[zz][r][(c4 + 3 + r) & 63] = v.w;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t qoff = (size_t)blockIdx.z * plane;  // float4 units
#pragma unroll 4
    for (int m = 0; m < 16; ++m) {
        const int r = w + 4 * m;  // a wave stores one 1 KiB run of a row per instruction
        const int s = (lane + r) & 63;
        if (bx + lane < n && by + r < n)
            nt_st4(xq + 4 * (qoff + (size_t)(by + r) * n + bx + lane), make_float4(t[0][r][s], t[1][r][s], t[2][r][s], t[3][r][s]));
    }
#pragma unroll 4
    for (int m = 0; m < 16; ++m) {
        const int r = w + 4 * m;  // column of the tile = row of the transposed copy
        const int s = (r + lane) & 63;
        if (bx + r < n && by + lane < n)
            nt_st4(xq_T + 4 * (qoff + (size_t)(bx + r) * n + by + lane), make_float4(t[0][lane][s], t[1][lane][s], t[2][lane][s], t[3][lane][s]));
    }
}

static inline bool aligned16(const void *a, const void *b, const void *c, const void *d)
{
#ifdef TOMO_GLUE32   // A/B builds only (tools/run_ab.sh): the 32 x 32 dword kernels everywhere
    return false;
#endif
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

template <bool LERP8, bool RESID>
__global__ __launch_bounds__(256) void fp_march_kernel(FpArgs a)
{
    constexpr int ZB = 4;
    const int iu = blockIdx.x * 256 + threadIdx.x;
    const int k_a = blockIdx.y;
    const int z0 = blockIdx.z * ZB;
    if (iu >= a.nu) return;
    const tomo_angle_t t = a.tab[k_a];
    const float half_n = 0.5f * (float)a.n - 0.5f, half_u = 0.5f * (float)a.nu - 0.5f;
    const float s = ((float)iu - half_u) + t.cor;
    const float offset = fmaf(s, t.inv, half_n);
    const float *src = t.dirx ? a.volT : a.vol;  // interpolation axis contiguous in either case
    const size_t zstride = (size_t)a.n * a.n;
    const int n = a.n;
    float acc[ZB] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float *base = src + (size_t)z0 * zstride;
    bool zok[ZB];
#pragma unroll
    for (int zz = 0; zz < ZB; ++zz) zok[zz] = z0 + zz < a.nz;
#pragma unroll 2
    for (int k = 0; k < n; ++k) {
        const float kw = (float)k - half_n;
        const float f = fmaf(kw, t.slope, offset);
        const float fl = floorf(f);
        const float w = lerp_w<LERP8>(f, fl), omw = 1.0f - w;
        const int i0 = (int)fl;
        const bool ok0 = (i0 >= 0) && (i0 < n), ok1 = (i0 + 1 >= 0) && (i0 + 1 < n);
        const float *row = base + (size_t)k * n;
#pragma unroll
        for (int zz = 0; zz < ZB; ++zz) {
            const float v0 = (ok0 && zok[zz]) ? row[zz * zstride + i0] : 0.0f;
            const float v1 = (ok1 && zok[zz]) ? row[zz * zstride + i0 + 1] : 0.0f;
            acc[zz] = fmaf(omw, v0, acc[zz]);
            acc[zz] = fmaf(w, v1, acc[zz]);
        }
    }
    float v4[ZB] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int zz = 0; zz < ZB; ++zz) {
        if (!zok[zz]) continue;
        const int z = z0 + zz;
        float val = acc[zz] * t.scale;
        if (RESID) val = fp_residual_value(a, val, z, k_a, t.src, iu);
        v4[zz] = val;
        if (!(RESID && a.zquad)) a.out[((size_t)z * a.na + k_a) * a.nu + iu] = val;
    }
    if (RESID && a.zquad)
        reinterpret_cast<float4 *>(a.out)[((size_t)(z0 >> 2) * a.na + k_a) * a.nu + iu] = make_float4(v4[0], v4[1], v4[2], v4[3]);
}

#include "fp_tiled.inl"

// The transposed-copy token: `of`'s in-plane transposed copy (quad-interleaved or planar) is in the context's scratch, good
// for exactly the next forward projection of `of` on stream `st`.
void volT_publish(tomo_ctx *ctx, const float *of, hipStream_t st, bool quad)
{
    ctx->volT_of = of;
    ctx->volT_stream = st;
    ctx->volT_quad = quad;
    ctx->volT_valid = true;
}

void volT_revoke(tomo_ctx *ctx)
{
    ctx->volT_valid = false;
    ctx->volT_of = nullptr;
}

// the context's in-plane transposed volume copy (x-stepping angles read it), grow-only: `slices` slices of the volume (nz, or
// whole quads for the quad-interleaved copy)
int fp_scratch(tomo_ctx *ctx, int slices)
{
    const size_t need = (size_t)slices * ctx->n * ctx->n * sizeof(float);
    if (ctx->scratch_bytes < need) {
        volT_revoke(ctx);
        if (ctx->scratch) { TOMO_HIP(hipDeviceSynchronize()); TOMO_HIP(hipFree(ctx->scratch)); ctx->scratch = nullptr; ctx->scratch_bytes = 0; }
        TOMO_HIP(hipMalloc(&ctx->scratch, need));
        ctx->scratch_bytes = need;
    }
    return TOMO_OK;
}

// ------------------------------------------------------------------------------------------ FP form selection (host)
// Every window bound the selection asks for depends on the geometry only: fp_tables computes them at context creation,
// fp_plan turns them into at most four launches (or the march) without a HIP call, and fp_run launches the plan.

// ---- per-angle lane -> pixel multiplier of the whole-row form (host).  Bank model of one ds_read_b128 service group: its 16
// lanes hold 16 consecutive logical positions t, i.e. pixels m*t mod bt, i.e. LDS slots floor(x0 + s*pixel) with s = 1/|cos|
// (|inv| of the angle record) in [1, 1.4143]; the LDS serves the group in as many cycles as the fullest of its 16 bank rows
// (slot mod 16) holds DIFFERENT slots.  m = 1 spans up to 22 slots (two-way conflicts: 1.5-2.0 cycles at 20-45 degrees), the
// best odd m < 64 per angle 1.5-1.7.  Measured on the kernel's own loop: tools/probes/fp_combo_probe.hip,
// profiles/r6_fp_combo_probe.txt (sampling loop x 1.09 alone, x 1.215 together with 8 slices per thread).
static double fp_bank_model(double s, int m, int bt)
{
    double total = 0.0;
    int cnt = 0;
    for (int ph = 0; ph < 8; ++ph) {
        const double x0 = 3.0 + ph * 0.91;
        for (int t0 = 0; t0 + 16 <= bt; t0 += 16 * 5) {   // every fifth service group
            int distinct[16], nd = 0, rows[16] = {0};
            for (int j = 0; j < 16; ++j) {
                const int slot = (int)std::floor(x0 + s * (double)((m * (t0 + j)) % bt));
                bool seen = false;
                for (int q = 0; q < nd; ++q) seen |= distinct[q] == slot;   // same slot: one broadcast
                if (!seen) { distinct[nd++] = slot; ++rows[slot & 15]; }
            }
            int worst = 1;
            for (int r = 0; r < 16; ++r) worst = std::max(worst, rows[r]);
            total += worst;
            ++cnt;
        }
    }
    return cnt ? total / cnt : 1.0;
}

// multiplier for stride s and tile width bt, memoised on a 1/512 grid of s (the model is smooth at that scale and a
// context asks for up to a few thousand angles)
static int fp_lane_mult(double s, int bt)
{
    static std::mutex mu;
    static std::map<std::pair<int, int>, int> memo;
    const int key = (int)std::lround((std::min(std::max(s, 1.0), 1.4143) - 1.0) * 512.0);
    std::lock_guard<std::mutex> lock(mu);
    auto it = memo.find({bt, key});
    if (it != memo.end()) return it->second;
    const double sq = 1.0 + key / 512.0;
    int best_m = 1;
    double best = fp_bank_model(sq, 1, bt);
    for (int m = 3; m < 64; m += 2) {
        if (std::gcd(m, bt) != 1) continue;   // m*t mod bt must be a bijection (bt = 896 = 2^7 * 7 rules out 7, 21, ...)
        const double c = fp_bank_model(sq, m, bt);
        if (c < best - 1e-3) { best = c; best_m = m; }
    }
    memo[{bt, key}] = best_m;
    return best_m;
}

// Upper bound (host, same float arithmetic as the kernel) of the staged window width over all groups / tiles / rows.
// The width is a max of affine functions of the row index minus a min of affine functions, hence convex: its maximum
// over the march is attained at the first or the last row.
static int fp_window_bound(const tomo_angle_t *tab, const int *order, int n_class, int n, int nu, int tile = 256,
                           int group = FP_A)
{
    const float half_n = 0.5f * (float)n - 0.5f, half_u = 0.5f * (float)nu - 0.5f;
    int bound = 2;
    const int nut = ceil_div(nu, tile);
    for (int g = 0; g * group < n_class; ++g) {
        const int ng = std::min(group, n_class - g * group);
        for (int ut = 0; ut < nut; ++ut) {
            for (int e = 0; e < 2; ++e) {
                const float kw = (float)(e ? n - 1 : 0) - half_n;
                float fmin = 3.0e38f, fmax = -3.0e38f;
                for (int i = 0; i < ng; ++i) {
                    const tomo_angle_t &t = tab[order[g * group + i]];
                    const float o0 = std::fmaf(((float)(ut * tile) - half_u) + t.cor, t.inv, half_n);
                    const float o1 = std::fmaf(((float)(ut * tile + tile - 1) - half_u) + t.cor, t.inv, half_n);
                    const float f0 = std::fmaf(kw, t.slope, o0), f1 = std::fmaf(kw, t.slope, o1);
                    fmin = std::min(fmin, std::min(f0, f1));
                    fmax = std::max(fmax, std::max(f0, f1));
                }
                // UNCLIPPED width: only that is convex in the row index (clipping to the volume can make the end rows
                // narrow while a middle row, fully inside the volume, is wide); the clip is applied once at the end
                const double wdt = (double)std::floor(fmax) + 1.0 - (double)std::floor(fmin) + 1.0;
                bound = std::max(bound, (int)std::min(wdt, (double)n + 4.0));
            }
        }
    }
    return std::min(bound + 2, n + 4);
}

constexpr int FP_A16 = 16;   // angles per workgroup of the dense form
// measured at 384..640-wide detectors (tools/kernel_bench.py): the whole-row form is 7-37 % faster than 256-pixel tiles
// there as well, so it is considered from 128 pixels up (it used to start at 768)
constexpr int FP_WIDE_MIN_NU = 128;
// lane multipliers, measured A/B (profiles/r6_fp_lane_multiplier_ab.txt): x 1.024 at 1024 pixels (configs[2]), x 1.047 at
// 896 (configs[4] share), 0.97-0.99 at 256-640 pixels where the un-permute of the epilogue is not paid back: from 768
// pixels up only
constexpr int FP_MULT_MIN_BT = 768;

// whole-row form: tiles of equal width: 2560 pixels = 3 tiles of 896 (14 waves), not 2.5 tiles of 1024
static int fp_wide_tiles(int nu) { return ceil_div(nu, 1024); }
static int fp_wide_bt(int nu) { return std::min(1024, ceil_div(ceil_div(nu, fp_wide_tiles(nu)), 64) * 64); }

enum FpForm { FP_WHOLE_ROW, FP_DENSE16, FP_TILED, FP_TILED_SYNC };

// one launch of the forward projector: the angles of one stepping class or, whole-row form up to 1024 pixels, of both
// sign classes of an axis
struct FpLaunch {
    FpForm form;
    int cls;              // stepping class (the first of a merged axis); x-stepping classes (cls >> 1) read the transposed volume
    bool merged;          // whole-row form: classes cls and cls + 1 in one launch
    size_t order_off;     // first entry in the order table (and in the lane-multiplier table)
    int n_angles;
    int wpitch;           // LDS pitch (float4) per staged row
    int threads;          // workgroup size = detector pixels per tile
    int passes, kc;       // column passes per staged row, rows per chunk
    int nut, ngroups;     // detector tiles, angle groups
    size_t lds;           // dynamic LDS bytes
    long blocks;
    bool mult;            // per-angle lane -> pixel multipliers (whole-row form)
    bool qv;              // whole-row double-buffered form staged by LDS-DMA from the quad-interleaved volume (TOMO_VOLUME_ZQUAD)
    int group;            // qv: angles per workgroup when not the form's own (0), see fp_plan_group13
};

struct FpPlan {
    bool march = false;   // the un-tiled march kernel over the whole subset instead
    bool qv = false;      // a quad-interleaved volume was asked for and EVERY launch reads it (fp_plan's `volq`)
    int count = 0;
    FpLaunch l[4];
};

static long fp_blocks(int nz, int nut, int ngroups) { return 8L * (((long)ceil_div(nz, 4) * nut * ngroups + 7) / 8); }

// Whole-row form (one workgroup per detector row tile, see fp_tiled.inl) for the `nc` angles at `off` of the order table,
// window `wp`.  Chosen when the 256-pixel tiles would stage at least 0.9x what whole rows need (cost_tiles) and it fits
// in LDS; false otherwise.
static bool fp_plan_whole_row(const tomo_ctx *ctx, int variant, int cls, bool merged, size_t off, int nc, int wp,
                              double cost_tiles, FpLaunch &l)
{
    const int nut = fp_wide_tiles(ctx->nu), bt = fp_wide_bt(ctx->nu);
    const double cost_rows = (double)nut * ceil_div(nc, FP_A) * wp;
    // measured: with equal staging volume the whole-row form is still the faster one (one workgroup per CU streams rows
    // through a deep prefetch pipeline; BASELINE configs[3], 1500 dense angles at 2048: 0.59 -> 0.51 s per ADMM
    // iteration), so it is taken whenever it does not stage clearly MORE than the 256-pixel tiles
    const bool pays = cost_tiles >= 0.9 * cost_rows;
    const int passes = ceil_div(wp, bt);
    // rows per chunk: 4 (or 2) double-buffered rows up to two column passes; detectors wider than 2048
    // (3-5 passes, BASELINE configs[4] is 2560 wide) keep ONE tile (two barriers per chunk) of as many
    // rows as fit in the 160 KiB of LDS next to the per-row window tables
    int kc = 4;
    const size_t tab = (size_t)ctx->n * 8;
    size_t lds = (size_t)2 * kc * wp * 16 + tab;
    if (passes <= 2) {
        if (lds > 160 * 1024) { kc = 2; lds = (size_t)2 * kc * wp * 16 + tab; }
    } else {
        kc = passes == 3 ? 2 : 1;  // 3 rows (9 float4 in flight per thread) spill at 1024 threads
        while (kc > 1 && (size_t)kc * wp * 16 + tab > 160 * 1024) --kc;
        lds = (size_t)kc * wp * 16 + tab;
    }
    if (!(pays && passes <= 5 && lds <= 160 * 1024)) return false;
    // per-angle lane -> pixel multipliers (round 6, fp_tables; variant 4, dev flavour: pixel = lane): the un-permute of
    // the epilogue needs two LDS rows of bt float4 inside the tile area
    const bool mult = bt >= FP_MULT_MIN_BT && (size_t)2 * bt * 16 <= lds - tab && variant != 4;
    l = {FP_WHOLE_ROW, cls, merged, off, nc, wp, bt, passes, kc, nut, ceil_div(nc, FP_A), lds,
         fp_blocks(ctx->nz, nut, ceil_div(nc, FP_A)), mult};
    return true;
}

// Dense form (round 4): 256 detector pixels x 16 angles per workgroup.  When neighbouring angles of the slope order are a
// fraction of a degree apart (BASELINE configs[3]: 1500 angles, no subsets) a 16-angle group's window is hardly wider
// than an 8-angle group's, so every staged volume row serves twice the rays: 0.12 staged columns per sample against
// 0.18 for whole rows x 8 angles.  Three 256-thread workgroups per CU (12 waves, <= 168 registers).  False where it
// does not apply.
static bool fp_plan_dense16(const tomo_ctx *ctx, const tomo_subset &s, int variant, int cls, size_t off, FpLaunch &l)
{
    const int nc = s.n_class[cls], wp = s.wbound16[cls];
    if (nc < 2 * FP_A16) return false;
    if (wp > 512) return false;  // two column passes at most
    const int passes = ceil_div(wp, 256);
    const int kc = passes == 1 ? 4 : 2;  // four float4 staging items per thread and chunk either way
    const size_t lds = (size_t)2 * kc * wp * 16 + (size_t)ctx->n * 8;
    if (lds > 64 * 1024) return false;  // three workgroups per CU
    const int nut = ceil_div(ctx->nu, 256), ngroups = ceil_div(nc, FP_A16);
    const long wgs = (long)ceil_div(ctx->nz, 4) * nut * ngroups;
    if (fp_blocks(ctx->nz, nut, ngroups) > 0x7fffffffL) return false;
    // a launch per sign class must still fill the chip several times over (768 resident workgroups): on BASELINE
    // configs[1] (256^3, 360 angles) the form left half the CUs idle -- 542 instead of 702 iterations/s
    if (wgs < 4 * 768 && variant != 3) return false;
    l = {FP_DENSE16, cls, false, off, nc, wp, 256, passes, kc, nut, ngroups, lds, fp_blocks(ctx->nz, nut, ngroups), false};
    return true;
}

// 256-pixel tiles x 8 angles for one class.  Windows of up to 1280 columns run the register-prefetch pipeline
// (double-buffered up to 512 columns, single-buffered beyond); wider ones (detectors wider than 1024 whose whole-row
// form does not fit in LDS) and variant 2 run the synchronous form: stage, barrier, sample, barrier, with a small LDS
// footprint so that several workgroups per CU hide the staging latency.
static FpLaunch fp_plan_tiled(const tomo_ctx *ctx, const tomo_subset &s, int variant, int cls, size_t off)
{
    const int nc = s.n_class[cls], wp = s.wbound[cls], nut = ceil_div(ctx->nu, 256), ngroups = ceil_div(nc, FP_A);
    const long blocks = fp_blocks(ctx->nz, nut, ngroups);
    const int passes = ceil_div(wp, 256);
    if (variant == 2 || wp > FP_MAX_WPITCH) {
        const int kc = std::max(1, std::min(8, 40000 / (wp * 16)));
        return {FP_TILED_SYNC, cls, false, off, nc, wp, 256, passes, kc, nut, ngroups, (size_t)kc * wp * 16, blocks, false};
    }
    // float4 staging items per thread and chunk (M = passes x rows per chunk) and double buffering, per pass count (1..5)
    const int m = passes <= 2 ? 8 : (passes == 5 ? 10 : 12);
    const int kc = m / passes;
    const size_t lds = (size_t)(passes <= 2 ? 2 : 1) * kc * wp * 16 + (size_t)ctx->n * 8;
    return {FP_TILED, cls, false, off, nc, wp, 256, passes, kc, nut, ngroups, lds, blocks, false};
}

// Angle groups sized to the class (round 7, qv launches only: the LDS-DMA staging leaves the registers for 13 x 4 accumulators
// under the 128 of a 1024-thread workgroup).  37 or 38 angles per axis (BASELINE configs[2]) make 3 groups of 13 -- 39 slots,
// 3 stagings of the volume -- instead of 5 groups of 8 -- 40 slots, 5 stagings.  Taken when 13-angle groups pad to no more
// slots than 8-angle groups do and the (wider) window still runs double-buffered.
constexpr int FP_A13 = 13;
static bool fp_plan_group13(const tomo_ctx *ctx, const tomo_subset &s, FpLaunch &l)
{
    if (ceil_div(l.n_angles, FP_A13) * FP_A13 > ceil_div(l.n_angles, FP_A) * FP_A) return false;
    const int wp = s.wbound_wide13[l.cls], passes = ceil_div(wp, l.threads);
    if (wp <= 0 || passes > 2) return false;
    const size_t tab = (size_t)ctx->n * 8;
    int kc = 4;
    size_t lds = (size_t)2 * kc * wp * 16 + tab;
    if (lds > 160 * 1024) { kc = 2; lds = (size_t)2 * kc * wp * 16 + tab; }
    if (lds > 160 * 1024) return false;
    l.wpitch = wp; l.passes = passes; l.kc = kc; l.lds = lds;
    l.ngroups = ceil_div(l.n_angles, FP_A13);
    l.blocks = fp_blocks(ctx->nz, l.nut, l.ngroups);
    l.mult = l.mult && (size_t)2 * l.threads * 16 <= lds - tab;
    l.group = FP_A13;
    return true;
}

// The forward projector's kernels for one subset (no HIP calls): per stepping axis the dense form or the whole-row form
// where they pay, 256-pixel tiles for every class left over, or the march when a class's window does not fit in LDS.
// `volq`: the caller holds the volume quad-interleaved (TOMO_VOLUME_ZQUAD).  Only the whole-row double-buffered form reads
// that layout, so the plan is marked `qv` when every launch takes it (BASELINE configs[2] and [4] do) and left planar --
// plan.qv false, for the caller to refuse -- otherwise.  Which forms are chosen does not depend on `volq`.
static int fp_plan(const tomo_ctx *ctx, const tomo_subset &s, int variant, FpPlan &plan, bool volq = false)
{
    // dense form taken when it stages <= 0.75x what whole rows x 8 angles would
    constexpr double FP_DENSE16_PAYS = 0.75;
    plan = FpPlan();
    // tiled forms unless a class's LDS window would not fit (very wide angular spread on a very wide volume): one staged
    // row must fit in 64 KiB of LDS
    plan.march = variant == 1;
    for (int c = 0; c < 4; ++c) plan.march |= s.n_class[c] > 0 && s.wbound[c] > 4000;
    if (plan.march) return TOMO_OK;
    const int nu = ctx->nu;
    size_t off[4] = {s.table_offset};
    for (int c = 1; c < 4; ++c) off[c] = off[c - 1] + s.n_class[c - 1];
    bool done[4] = {false, false, false, false};
    for (int d = 0; d < 2 && (variant == 0 || variant == 3 || variant == 4) && nu >= FP_WIDE_MIN_NU; ++d) {
        const int c0 = 2 * d, c1 = c0 + 1, nc0 = s.n_class[c0], nc1 = s.n_class[c1], nc = nc0 + nc1;
        if (nc == 0) continue;
        // dense form for both sign classes of the axis when it stages clearly less than whole rows x 8 angles would
        // (variant 3, dev flavour: whenever it is applicable -- the A/B and parity tests of this form)
        FpLaunch e0, e1;
        bool take = (nc0 == 0 || fp_plan_dense16(ctx, s, variant, c0, off[c0], e0)) &&
                    (nc1 == 0 || fp_plan_dense16(ctx, s, variant, c1, off[c1], e1));
        if (take && variant != 3) {
            const double cost = (nc0 ? (double)e0.nut * e0.ngroups * e0.wpitch : 0.0) +
                                (nc1 ? (double)e1.nut * e1.ngroups * e1.wpitch : 0.0);
            const int nut_w = fp_wide_tiles(nu);
            const double rows = nu <= 1024 ? (double)nut_w * ceil_div(nc, FP_A) * s.wbound_wide[c0]
                                           : (double)nut_w * ceil_div(nc0, FP_A) * s.wbound_wide[c0] +
                                             (double)nut_w * ceil_div(nc1, FP_A) * s.wbound_wide[c1];
            take = cost <= FP_DENSE16_PAYS * rows;
        }
        if (take) {
            if (nc0) plan.l[plan.count++] = e0;
            if (nc1) plan.l[plan.count++] = e1;
            done[c0] = done[c1] = true;
            continue;
        }
        if (variant == 3) continue;
        const int nut = ceil_div(nu, 256);
        const double ct0 = (double)nut * ceil_div(nc0, FP_A) * s.wbound[c0];
        const double ct1 = (double)nut * ceil_div(nc1, FP_A) * s.wbound[c1];
        FpLaunch l;
        if (nu <= 1024) {
            // one 1024-pixel tile = the whole detector row: its window does not care about the sign of the detector
            // slope, so the two classes of an axis (adjacent in the order table) are merged -- 37 angles make 5 groups
            // of 8 instead of 3 + 3
            if (fp_plan_whole_row(ctx, variant, c0, true, off[c0], nc, s.wbound_wide[c0], ct0 + ct1, l)) {
                plan.l[plan.count++] = l;
                done[c0] = done[c1] = true;
            }
        } else {
            // several 1024-pixel tiles per row (2560-wide detectors, BASELINE configs[4]): a group that mixes the two
            // signs of the slope maps a tile to BOTH ends of the volume row (window = the whole row, 2564 columns for
            // every tile); class by class a tile's window stays ~1400 columns
            for (int c = c0; c <= c1; ++c)
                if (s.n_class[c] > 0 && fp_plan_whole_row(ctx, variant, c, false, off[c], s.n_class[c], s.wbound_wide[c],
                                                          c == c0 ? ct0 : ct1, l)) {
                    plan.l[plan.count++] = l;
                    done[c] = true;
                }
        }
    }
    for (int c = 0; c < 4; ++c)  // one launch per stepping class (x-stepping classes read the transposed copy)
        if (s.n_class[c] > 0 && !done[c]) plan.l[plan.count++] = fp_plan_tiled(ctx, s, variant, c, off[c]);
    for (int i = 0; i < plan.count; ++i) {
        TOMO_REQUIRE(plan.l[i].blocks <= 0x7fffffffL, "problem too large for one FP launch");
        TOMO_REQUIRE(plan.l[i].form != FP_TILED_SYNC || plan.l[i].lds <= 64 * 1024,
                     "forward-projection window does not fit in LDS");
    }
    if (volq && ctx->n % 4 == 0) {
        plan.qv = plan.count > 0;
        for (int i = 0; i < plan.count; ++i) plan.qv &= plan.l[i].form == FP_WHOLE_ROW && plan.l[i].passes <= 2;
        for (int i = 0; i < plan.count; ++i) plan.l[i].qv = plan.qv;
        for (int i = 0; i < plan.count && plan.qv; ++i) (void)fp_plan_group13(ctx, s, plan.l[i]);
    }
    return TOMO_OK;
}

// what one launch contributes to tomo_ctx_kernel_path("fp")
static std::string fp_path_text(const FpLaunch &l)
{
    const std::string cls = "class" + std::to_string(l.cls) + ":", passes = std::to_string(l.passes) + " passes";
    switch (l.form) {
    case FP_WHOLE_ROW:
        return std::string(l.cls >> 1 ? "x" : "y") + (l.merged ? "" : (l.cls & 1) ? "-" : "+") + ":whole-row(" +
               std::to_string(l.threads) + " threads, " + passes + ", " + std::to_string(l.kc) + " rows/chunk" +
               (l.qv ? ", quad-interleaved volume, LDS-DMA staging" + std::string(l.group ? ", " + std::to_string(l.group) + " angles) " : ") ")
                     : ") ");
    case FP_DENSE16: return cls + "dense(256 pixels x 16 angles, " + passes + ") ";
    case FP_TILED: return cls + "tiled-pipelined(256 threads, " + passes + ") ";
    default: return cls + "tiled-sync(window " + std::to_string(l.wpitch) + ") ";
    }
}

// The kernel instantiation that serves a plan entry -- (form, column passes, float4 staging items per thread and chunk
// = passes x rows per chunk; double-buffered tile up to two passes) -- launched.
template <bool L8, bool RES>
static void fp_launch(const FpLaunch &l, const FpTiledArgs &t, hipStream_t st)
{
    using Kernel = void (*)(FpTiledArgs);
    const int m = l.passes * l.kc;
    Kernel k;
    switch (l.form) {
    case FP_TILED_SYNC:
        fp_tiled_sync_kernel<L8, RES, 256, FP_A><<<(unsigned)l.blocks, 256, l.lds, st>>>(t, l.kc);
        return;
    case FP_WHOLE_ROW:   // the 1024-thread instantiations, launched with l.threads <= 1024
        if (l.qv && l.group == FP_A13 && l.passes == 1) k = fp_tiled_kernel<L8, RES, 1, 4, true, 1024, FP_A13, true>;
        else if (l.qv && l.group == FP_A13 && m == 8) k = fp_tiled_kernel<L8, RES, 2, 8, true, 1024, FP_A13, true>;
        else if (l.qv && l.group == FP_A13) k = fp_tiled_kernel<L8, RES, 2, 4, true, 1024, FP_A13, true>;
        else if (l.qv && l.passes == 1) k = fp_tiled_kernel<L8, RES, 1, 4, true, 1024, FP_A, true>;
        else if (l.qv && m == 8) k = fp_tiled_kernel<L8, RES, 2, 8, true, 1024, FP_A, true>;
        else if (l.qv) k = fp_tiled_kernel<L8, RES, 2, 4, true, 1024, FP_A, true>;
        else if (l.passes == 1) k = fp_tiled_kernel<L8, RES, 1, 4, true, 1024>;
        else if (l.passes == 2 && m == 8) k = fp_tiled_kernel<L8, RES, 2, 8, true, 1024>;
        else if (l.passes == 2) k = fp_tiled_kernel<L8, RES, 2, 4, true, 1024>;
        else if (l.passes == 3 && m == 6) k = fp_tiled_kernel<L8, RES, 3, 6, false, 1024>;
        else if (l.passes == 3) k = fp_tiled_kernel<L8, RES, 3, 3, false, 1024>;
        else if (l.passes == 4) k = fp_tiled_kernel<L8, RES, 4, 4, false, 1024>;
        else k = fp_tiled_kernel<L8, RES, 5, 5, false, 1024>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds);
        break;
    case FP_DENSE16:
        if (l.passes == 1) k = fp_tiled_kernel<L8, RES, 1, 4, true, 256, FP_A16>;
        else k = fp_tiled_kernel<L8, RES, 2, 4, true, 256, FP_A16>;
        break;
    default:
        if (l.passes == 1) k = fp_tiled_kernel<L8, RES, 1, 8, true, 256>;
        else if (l.passes == 2) k = fp_tiled_kernel<L8, RES, 2, 8, true, 256>;
        else if (l.passes == 3) k = fp_tiled_kernel<L8, RES, 3, 12, false, 256>;
        else if (l.passes == 4) k = fp_tiled_kernel<L8, RES, 4, 12, false, 256>;
        else k = fp_tiled_kernel<L8, RES, 5, 10, false, 256>;
    }
    k<<<(unsigned)l.blocks, l.threads, l.lds, st>>>(t);
}

int fp_run(tomo_ctx *ctx, int subset, const float *vol, const float *b, const float *w, int gathered, int fidelity,
           float *out, void *stream, const float *ring = nullptr, float ring_scale = 0.0f, int zquad = 0,
           int robust = TOMO_ROBUST_NONE, float rdelta = 0.0f, int volq = 0)
{
    TOMO_REQUIRE(ctx != nullptr, "ctx is NULL");
    TOMO_REQUIRE(vol != nullptr && out != nullptr, "NULL data pointer");
    TOMO_REQUIRE(subset < ctx->os, "subset %d out of range (OS_number %d)", subset, ctx->os);
    const tomo_subset &s = *find_subset(ctx, subset);
    hipStream_t st = as_stream(stream);
    // the transposed copy tomo_momentum_transposed left behind is a ONE-SHOT token: whatever this call does with it
    // (use it, find it belongs to another volume / stream, return early), it is spent before anything else happens
    const bool ready = ctx->volT_valid && ctx->volT_of == vol && ctx->volT_stream == st && ctx->scratch != nullptr &&
                       ctx->volT_quad == (volq != 0);
    volT_revoke(ctx);
    if (s.size == 0) return TOMO_OK;
    TOMO_ON_DEVICE(ctx->device);
    // fp variant 5 (both flavours) only makes tomo_ctx_volume_zquad_ok say no, so that a driver keeps the planar volume (A/B)
    const int variant = g_variant_fp == 5 ? 0 : g_variant_fp;
    FpArgs a;
    a.vol = vol;
    a.volT = nullptr;
    if (volq) {
        // `vol` is the quad-interleaved volume; its in-plane transposed twin is the token the producer (tomo_momentum_transposed
        // or tomo_volume_to_zquad) has just left in the context.  Nothing here converts: the layout exists to spare that pass.
        TOMO_REQUIRE((((uintptr_t)vol) & 15) == 0, "the quad-interleaved volume must be 16-byte aligned");
        TOMO_REQUIRE(s.n_dirx == 0 || ready, "a quad-interleaved volume is forward projected once, right after tomo_momentum_transposed / "
                                             "tomo_volume_to_zquad wrote it on the same stream");
        a.volT = (const float *)ctx->scratch;
    } else if (s.n_dirx > 0) {
        int rc = fp_scratch(ctx, ctx->nz);
        if (rc != TOMO_OK) return rc;
        // tomo_momentum_transposed has just written this volume's transposed copy: use it once, skip the pass
        if (!ready) {
            if (ctx->n % 4 == 0 && aligned16(vol, ctx->scratch, nullptr, nullptr)) {
                dim3 tg(ceil_div(ctx->n, 64), ceil_div(ctx->n, 64), ctx->nz);
                transpose64_kernel<false><<<tg, 256, 0, st>>>(vol, nullptr, nullptr, (float *)ctx->scratch, 0.0f, ctx->n);
            } else {
                dim3 tg(ceil_div(ctx->n, 32), ceil_div(ctx->n, 32), ctx->nz);
                momentum_transpose_kernel<false><<<tg, 256, 0, st>>>(vol, nullptr, nullptr, (float *)ctx->scratch, 0.0f, ctx->n);
            }
            TOMO_LAUNCH_CHECK();
        }
        a.volT = (const float *)ctx->scratch;
    }
    a.tab = ctx->dev_table + s.table_offset;
    a.nz = ctx->nz; a.n = ctx->n; a.nu = ctx->nu; a.na = s.size; a.na_full = ctx->na;
    a.out = out; a.b = b; a.w = w; a.fidelity = fidelity; a.gathered = gathered;
    a.ring = ring; a.ring_scale = ring_scale;
    a.robust = (b != nullptr) ? robust : TOMO_ROBUST_NONE; a.rdelta = rdelta;
    a.zquad = (b != nullptr) ? zquad : 0;
    if (a.zquad && (((uintptr_t)out) & 15) != 0)
        return tomo_fail(TOMO_E_INVALID, "the quad-interleaved residual must be 16-byte aligned");
    tomo_prof_scope prof(PROF_FP, st, 1);
    ctx->last_fp_path.clear();
    const bool l8 = (ctx->flags & TOMO_FLAG_LERP8) != 0;
    FpPlan plan;
    const int rc = fp_plan(ctx, s, variant, plan, volq != 0);
    if (rc != TOMO_OK) return rc;
    TOMO_REQUIRE(!volq || plan.qv, "this subset's forward projection does not read the quad-interleaved volume "
                                   "(tomo_ctx_volume_zquad_ok says so beforehand)");
    if (plan.march) {
        ctx->last_fp_path = "march(no LDS)";
        if (variant != 1) tomo_warn_once("fp_march", "forward projection: a staged row window exceeds 64 KiB of LDS, "
                                              "falling back to the un-tiled march kernel (about 4x slower)");
        dim3 grid(ceil_div(ctx->nu, 256), s.size, ceil_div(ctx->nz, 4));
        if (b) {
            if (l8) fp_march_kernel<true, true><<<grid, 256, 0, st>>>(a);
            else fp_march_kernel<false, true><<<grid, 256, 0, st>>>(a);
        } else {
            if (l8) fp_march_kernel<true, false><<<grid, 256, 0, st>>>(a);
            else fp_march_kernel<false, false><<<grid, 256, 0, st>>>(a);
        }
        TOMO_LAUNCH_CHECK();
        return TOMO_OK;
    }
    FpTiledArgs t;
    t.tab = a.tab;
    t.nz = a.nz; t.n = a.n; t.nu = a.nu; t.na = a.na; t.na_full = a.na_full;
    t.out = out; t.b = b; t.w = w; t.fidelity = fidelity; t.gathered = gathered;
    t.ring = ring; t.ring_scale = ring_scale; t.zquad = a.zquad; t.robust = a.robust; t.rdelta = a.rdelta;
#if TOMO_DEV
    t.probe = g_probe;
#endif
    t.nzb = ceil_div(a.nz, 4);
    for (int i = 0; i < plan.count; ++i) {
        const FpLaunch &l = plan.l[i];
        t.src = (l.cls >> 1) ? a.volT : a.vol;
        t.order = ctx->dev_fp_order + l.order_off;
        t.mult = l.mult ? ctx->dev_fp_mult + l.order_off : nullptr;
        t.n_class = l.n_angles; t.wpitch = l.wpitch; t.nut = l.nut; t.bt = l.threads; t.ngroups = l.ngroups;
        if (b) { if (l8) fp_launch<true, true>(l, t, st); else fp_launch<false, true>(l, t, st); }
        else   { if (l8) fp_launch<true, false>(l, t, st); else fp_launch<false, false>(l, t, st); }
        TOMO_LAUNCH_CHECK();
        ctx->last_fp_path += fp_path_text(l);
    }
    return TOMO_OK;
}

}  // namespace

// The forward projector's window bounds of every subset and the whole-row form's lane-multiplier table (tomo_ctx_create):
// both depend on the geometry only, so fp_plan reads them without a HIP call.
int fp_tables(tomo_ctx *ctx)
{
    const int n = ctx->n, nu = ctx->nu, bt = fp_wide_bt(nu);
    for (tomo_subset &s : ctx->subsets) {
        const tomo_angle_t *tab = ctx->host_table.data() + s.table_offset;
        const int *order = ctx->host_fp_order.data() + s.table_offset;
        for (int d = 0, off = 0; d < 2; ++d) {
            const int nc0 = s.n_class[2 * d], nc1 = s.n_class[2 * d + 1];
            for (int h = 0; h < 2; ++h) {
                const int c = 2 * d + h, nc = h ? nc1 : nc0, o = off + (h ? nc0 : 0);
                if (nc == 0) continue;
                s.wbound[c] = fp_window_bound(tab, order + o, nc, n, nu);
                s.wbound16[c] = fp_window_bound(tab, order + o, nc, n, nu, 256, FP_A16);
                if (nu > 1024) s.wbound_wide[c] = fp_window_bound(tab, order + o, nc, n, nu, bt);
                if (nu > 1024) s.wbound_wide13[c] = fp_window_bound(tab, order + o, nc, n, nu, bt, FP_A13);
            }
            if (nu <= 1024 && nc0 + nc1 > 0) s.wbound_wide[2 * d] = fp_window_bound(tab, order + off, nc0 + nc1, n, nu, bt);
            if (nu <= 1024 && nc0 + nc1 > 0) s.wbound_wide13[2 * d] = fp_window_bound(tab, order + off, nc0 + nc1, n, nu, bt, FP_A13);
            off += nc0 + nc1;
        }
    }
    if (bt < FP_MULT_MIN_BT) return TOMO_OK;
    std::vector<int> mult(ctx->host_fp_order.size(), 1);
    for (const tomo_subset &s : ctx->subsets)
        for (int i = 0; i < s.size; ++i) {
            const tomo_angle_t &rec = ctx->host_table[s.table_offset + ctx->host_fp_order[s.table_offset + i]];
            mult[s.table_offset + i] = fp_lane_mult(std::fabs((double)rec.inv), bt);
        }
    TOMO_HIP(hipMalloc((void **)&ctx->dev_fp_mult, std::max<size_t>(mult.size(), 1) * sizeof(int)));
    TOMO_HIP(hipMemcpy(ctx->dev_fp_mult, mult.data(), mult.size() * sizeof(int), hipMemcpyHostToDevice));
    return TOMO_OK;
}

void tomo_bp_relay_reset(int device)
{
    if (device < 0 || device >= BP_RELAY_DEVICES) return;
    g_bp_relay[device].refused.store(~(size_t)0);
    g_bp_relay[device].skipped.store(0);
}

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" int tomo_fp3d(tomo_ctx *ctx, int subset, const float *vol_dev, float *sino_dev, void *stream)
{
    return fp_run(ctx, subset, vol_dev, nullptr, nullptr, 0, TOMO_FID_LS, sino_dev, stream);
}

extern "C" int tomo_fp3d_residual(tomo_ctx *ctx, int subset, const float *vol_dev, const float *b_full_dev,
                                  const float *w_full_dev, int gathered, int fidelity, float *res_dev, void *stream)
{
    TOMO_REQUIRE(b_full_dev != nullptr, "projection data pointer is NULL");
    TOMO_REQUIRE(fidelity == TOMO_FID_LS || fidelity == TOMO_FID_PWLS || fidelity == TOMO_FID_KL ||
                     fidelity == TOMO_FID_RATIO,
                 "data_fidelity should be LS, PWLS or KL");
    TOMO_REQUIRE(fidelity != TOMO_FID_PWLS || w_full_dev != nullptr, "PWLS needs the weights");
    return fp_run(ctx, subset, vol_dev, b_full_dev, fidelity == TOMO_FID_PWLS ? w_full_dev : nullptr, gathered,
                  fidelity, res_dev, stream, nullptr, 0.0f, ctx ? ctx->res_layout : 0, TOMO_ROBUST_NONE, 0.0f,
                  ctx ? ctx->vol_layout : 0);
}

extern "C" int tomo_fp3d_residual_robust(tomo_ctx *ctx, int subset, const float *vol_dev, const float *b_full_dev,
                                         const float *w_full_dev, int gathered, int fidelity, int robust, float delta,
                                         float *res_dev, void *stream)
{
    TOMO_REQUIRE(b_full_dev != nullptr, "projection data pointer is NULL");
    TOMO_REQUIRE(fidelity == TOMO_FID_LS || fidelity == TOMO_FID_PWLS, "the Huber / Student's-t re-weighting applies to the LS and PWLS residuals");
    TOMO_REQUIRE(fidelity != TOMO_FID_PWLS || w_full_dev != nullptr, "PWLS needs the weights");
    TOMO_REQUIRE(robust == TOMO_ROBUST_NONE || robust == TOMO_ROBUST_HUBER || robust == TOMO_ROBUST_STUDENTST, "unknown robust mode %d", robust);
    TOMO_REQUIRE(robust == TOMO_ROBUST_NONE || delta > 0.0f, "the Huber / Student's-t threshold must be positive");
    return fp_run(ctx, subset, vol_dev, b_full_dev, fidelity == TOMO_FID_PWLS ? w_full_dev : nullptr, gathered,
                  fidelity, res_dev, stream, nullptr, 0.0f, ctx ? ctx->res_layout : 0, robust, delta, ctx ? ctx->vol_layout : 0);
}

extern "C" int tomo_ctx_set_residual_layout(tomo_ctx *ctx, int layout)
{
    TOMO_REQUIRE(ctx != nullptr, "ctx is NULL");
    TOMO_REQUIRE(layout == TOMO_RESIDUAL_PLANAR || layout == TOMO_RESIDUAL_ZQUAD, "unknown residual layout %d", layout);
    ctx->res_layout = layout;
    return TOMO_OK;
}

extern "C" int tomo_ctx_residual_layout(const tomo_ctx *ctx) { return ctx ? ctx->res_layout : -1; }

extern "C" size_t tomo_ctx_residual_elems(const tomo_ctx *ctx, int subset)
{
    if (!ctx || subset >= ctx->os) return 0;
    const tomo_subset &s = *find_subset(ctx, subset);
    const size_t nzr = ctx->res_layout == TOMO_RESIDUAL_ZQUAD ? (size_t)ceil_div(ctx->nz, 4) * 4 : (size_t)ctx->nz;
    return nzr * (size_t)s.size * (size_t)ctx->nu;
}

// ---- private volume layout (TOMO_VOLUME_ZQUAD, tomo_mi355x.h)
extern "C" int tomo_ctx_set_volume_layout(tomo_ctx *ctx, int layout)
{
    TOMO_REQUIRE(ctx != nullptr, "ctx is NULL");
    TOMO_REQUIRE(layout == TOMO_VOLUME_PLANAR || layout == TOMO_VOLUME_ZQUAD, "unknown volume layout %d", layout);
    TOMO_REQUIRE(layout == TOMO_VOLUME_PLANAR || ctx->n % 4 == 0, "the quad-interleaved volume needs a slice size that is a multiple of 4");
    ctx->vol_layout = layout;
    volT_revoke(ctx);   // a token of the other layout is worth nothing
    return TOMO_OK;
}

extern "C" int tomo_ctx_volume_layout(const tomo_ctx *ctx) { return ctx ? ctx->vol_layout : -1; }

extern "C" size_t tomo_ctx_volume_elems(const tomo_ctx *ctx)
{
    if (!ctx) return 0;
    const size_t nzv = ctx->vol_layout == TOMO_VOLUME_ZQUAD ? (size_t)ceil_div(ctx->nz, 4) * 4 : (size_t)ctx->nz;
    return nzv * (size_t)ctx->n * (size_t)ctx->n;
}

// Would subset `subset` run on a quad-interleaved X_t?  Host arithmetic only.  Yes when the forward projector plans the
// whole-row double-buffered form for every launch and the back projector's brick kernel (whose epilogue reads the layout)
// serves the subset; no under fp variant 5, the A/B switch that keeps a driver on the planar volume.
extern "C" int tomo_ctx_volume_zquad_ok(const tomo_ctx *ctx, int subset)
{
    if (!ctx || subset >= ctx->os || ctx->n % 4 != 0 || ceil_div(ctx->nz, 4) > 65535) return 0;
    if (g_variant_fp != 0 || (g_variant_bp != 0 && g_variant_bp != 3)) return 0;
    const tomo_subset &s = *find_subset(ctx, subset);
    if (s.size == 0 || (long)s.size * ctx->nu >= (1L << 25)) return 0;
    FpPlan plan;
    if (fp_plan(ctx, s, 0, plan, true) != TOMO_OK) return 0;
    return plan.qv ? 1 : 0;
}

// x (planar), optionally with the momentum of xold, -> xq and the transposed token in the context's scratch
static int volume_zquad_produce(tomo_ctx *ctx, const float *x_dev, const float *xold_dev, float *xq_dev, float beta, void *stream)
{
    TOMO_REQUIRE(ctx->n % 4 == 0 && aligned16(x_dev, xold_dev, xq_dev, nullptr),
                 "the quad-interleaved volume needs a slice size that is a multiple of 4 and 16-byte aligned arrays");
    const int nq = ceil_div(ctx->nz, 4);
    TOMO_REQUIRE(nq <= 65535, "too many slices for one launch");
    TOMO_ON_DEVICE(ctx->device);
    int rc = fp_scratch(ctx, 4 * nq);  // whole quads
    if (rc != TOMO_OK) return rc;
    dim3 tg(ceil_div(ctx->n, 64), ceil_div(ctx->n, 64), nq);
    if (xold_dev) zquad64_kernel<true><<<tg, 256, 0, as_stream(stream)>>>(x_dev, xold_dev, xq_dev, (float *)ctx->scratch, beta, ctx->n, ctx->nz);
    else zquad64_kernel<false><<<tg, 256, 0, as_stream(stream)>>>(x_dev, nullptr, xq_dev, (float *)ctx->scratch, 0.0f, ctx->n, ctx->nz);
    TOMO_LAUNCH_CHECK();
    volT_publish(ctx, xq_dev, as_stream(stream), true);
    return TOMO_OK;
}

extern "C" int tomo_volume_to_zquad(tomo_ctx *ctx, const float *x_dev, float *xq_dev, void *stream)
{
    TOMO_REQUIRE(ctx != nullptr && x_dev && xq_dev, "NULL argument");
    return volume_zquad_produce(ctx, x_dev, nullptr, xq_dev, 0.0f, stream);
}

extern "C" int tomo_momentum_transposed(tomo_ctx *ctx, const float *x_dev, const float *xold_dev, float *xt_dev, float beta,
                                        void *stream)
{
    TOMO_REQUIRE(ctx != nullptr && x_dev && xold_dev && xt_dev, "NULL argument");
    if (ctx->vol_layout == TOMO_VOLUME_ZQUAD) return volume_zquad_produce(ctx, x_dev, xold_dev, xt_dev, beta, stream);
    TOMO_ON_DEVICE(ctx->device);
    int rc = fp_scratch(ctx, ctx->nz);
    if (rc != TOMO_OK) return rc;
    if (ctx->n % 4 == 0 && aligned16(x_dev, xold_dev, xt_dev, ctx->scratch)) {
        dim3 tg(ceil_div(ctx->n, 64), ceil_div(ctx->n, 64), ctx->nz);
        transpose64_kernel<true><<<tg, 256, 0, as_stream(stream)>>>(x_dev, xold_dev, xt_dev, (float *)ctx->scratch, beta, ctx->n);
    } else {
        dim3 tg(ceil_div(ctx->n, 32), ceil_div(ctx->n, 32), ctx->nz);
        momentum_transpose_kernel<true><<<tg, 256, 0, as_stream(stream)>>>(x_dev, xold_dev, xt_dev, (float *)ctx->scratch, beta, ctx->n);
    }
    TOMO_LAUNCH_CHECK();
    volT_publish(ctx, xt_dev, as_stream(stream), false);
    return TOMO_OK;
}

extern "C" int tomo_ctx_invalidate(tomo_ctx *ctx)
{
    TOMO_REQUIRE(ctx != nullptr, "ctx is NULL");
    volT_revoke(ctx);
    return TOMO_OK;
}

extern "C" int tomo_fp3d_residual_ring(tomo_ctx *ctx, int subset, const float *vol_dev, const float *b_full_dev,
                                       const float *ring_dev, float ring_scale, float *res_dev, void *stream)
{
    TOMO_REQUIRE(b_full_dev != nullptr && ring_dev != nullptr, "projection data / ring offset pointer is NULL");
    TOMO_REQUIRE(ctx == nullptr || ctx->res_layout == TOMO_RESIDUAL_PLANAR,
                 "the ring-term residual is read by tomo_ring_gh_reduce in the planar layout: set TOMO_RESIDUAL_PLANAR first");
    TOMO_REQUIRE(ctx == nullptr || ctx->vol_layout == TOMO_VOLUME_PLANAR, "the ring-term residual takes the planar volume: set TOMO_VOLUME_PLANAR first");
    return fp_run(ctx, subset, vol_dev, b_full_dev, nullptr, 0, TOMO_FID_LS, res_dev, stream, ring_dev, ring_scale);
}

// ---- the voxel-driven back projector's entry points: bp_prepare, the form's filler (bp_common.h), the layout flags, bp_launch
extern "C" int tomo_bp3d(tomo_ctx *ctx, int subset, const float *sino_dev, float *vol_dev, void *stream)
{
    BpArgs a;
    int rc = bp_prepare(ctx, subset, sino_dev, a);
    if (rc == TOMO_OK) rc = bp_fill_plain(a, vol_dev);
    if (rc != TOMO_OK) return rc;
    return bp_launch<EPI_PLAIN>(a, (ctx->flags & TOMO_FLAG_LERP8) != 0, as_stream(stream));
}

extern "C" int tomo_bp3d_fista(tomo_ctx *ctx, int subset, const float *res_dev, const float *xt_dev,
                               float *xout_dev, float l_inv, int nonneg, void *stream)
{
    BpArgs a;
    int rc = bp_prepare(ctx, subset, res_dev, a);
    if (rc == TOMO_OK) rc = bp_fill_fista(a, xt_dev, xout_dev, l_inv, nonneg);
    if (rc != TOMO_OK) return rc;
    a.zquad = ctx->res_layout == TOMO_RESIDUAL_ZQUAD;
    a.xt_zquad = ctx->vol_layout == TOMO_VOLUME_ZQUAD;
    return bp_launch<EPI_FISTA>(a, (ctx->flags & TOMO_FLAG_LERP8) != 0, as_stream(stream));
}

extern "C" int tomo_bp3d_fista_momentum(tomo_ctx *ctx, int subset, const float *res_dev, float *xt_dev,
                                        float *xold_x_dev, float l_inv, float beta, int nonneg, void *stream)
{
    BpArgs a;
    int rc = bp_prepare(ctx, subset, res_dev, a);
    if (rc == TOMO_OK) rc = bp_fill_fista_momentum(a, xt_dev, xold_x_dev, l_inv, beta, nonneg);
    if (rc != TOMO_OK) return rc;
    TOMO_REQUIRE(ctx->vol_layout == TOMO_VOLUME_PLANAR, "the fused gradient step + momentum takes the planar volume: set TOMO_VOLUME_PLANAR first");
    a.zquad = ctx->res_layout == TOMO_RESIDUAL_ZQUAD;
    return bp_launch<EPI_FISTA_MOM>(a, (ctx->flags & TOMO_FLAG_LERP8) != 0, as_stream(stream));
}

extern "C" int tomo_bp3d_admm(tomo_ctx *ctx, int subset, const float *res_dev, float *z_dev, const float *x_dev,
                              const float *u_dev, float *zu_out_dev, float tau, float rho, int relax_on,
                              float one_minus_alpha, float alpha, int nonneg, void *stream)
{
    BpArgs a;
    int rc = bp_prepare(ctx, subset, res_dev, a);
    if (rc == TOMO_OK) rc = bp_fill_admm(a, z_dev, x_dev, u_dev, zu_out_dev, tau, rho, relax_on, one_minus_alpha, alpha, nonneg);
    if (rc != TOMO_OK) return rc;
    TOMO_REQUIRE(ctx->vol_layout == TOMO_VOLUME_PLANAR, "the ADMM z-update takes the planar volume: set TOMO_VOLUME_PLANAR first");
    a.zquad = ctx->res_layout == TOMO_RESIDUAL_ZQUAD;
    return bp_launch<EPI_ADMM>(a, (ctx->flags & TOMO_FLAG_LERP8) != 0, as_stream(stream));
}
