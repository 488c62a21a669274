// The three convolutions of the PrimX VAE ENCODER that the decoder's kernels do not cover (models/vae3d_dib.py:270-327,
// 431-435): conv_in (6 -> 32 on the fp32 channel-first 8^3 payload), the stride-2 downsample of
// down_blocks[0] (32 -> 32, 8^3 -> 4^3) and the head (conv_out 256 -> 2 on the 4^3 grid followed by quant_conv 2 -> 2).
// Everything between them runs on the decoder's entry points (conv3s8c32.hip, conv3.hip, gemm.hip, attention.hip, vae.hip).
//
// All three are activation-resident like conv3s8c32.hip: a persistent workgroup reads one primitive into LDS once, a tap
// is an address offset, and the next primitive's rows arrive in registers under the arithmetic.  Per-primitive offsets
// are 64-bit.
//
//   enc_conv_in_kernel   fp32 [P, 6, 512] -> 16-bit [P, 512, 32].  The layout change, the optional normalisation (channel
//                        0 * 5, the others * 2 - 1: the inverse of primx_vae_output(denorm)) and the rounding to 16 bits
//                        happen on the way into LDS: a zero-haloed 10^3 volume of 16-byte rows (6 channels + 2 zeros).
//                        One k-chunk of a 16x16x32 MFMA is then ONE TAP: lane group q reads the row of tap 4 s + q, 7
//                        steps cover the 27 taps (the 28th has zero weights and re-reads the centre row).  The weight
//                        fragments (7 x 2 x 8 values per lane) are gathered once per workgroup from the [32, Kpad]
//                        k = tap * 6 + ci form and stay in registers.  Bound by reading 12 KB and writing 32 KB.
//   conv3_down_kernel    16-bit [P, 512, 32] -> [P, 64, 32], stride 2, pad 1: output o reads inputs 2 o - 1 .. 2 o + 1, so
//                        only the low halo is ever touched.  Volume layout, swizzle and weight image are those of
//                        conv3_s8c32_kernel (primx_conv3d_s8c32_pack makes the image); wave w owns output plane w >> 1
//                        (16 voxels) and the 16 output channels of image half w & 1: 27 MFMAs.  Bound by the 32 KB read.
//   enc_head_kernel      16-bit [P, 64, 256] -> fp32 [P, 2, 64].  N = 2 would waste 15/16 of an MFMA tile: a dot-product
//                        kernel.  Thread = (row of 4 output voxels along x, 8-channel chunk); per (dz, dy) it reads the 4
//                        input voxels of the row and the 3 x 2 weight vectors once (16 MACs per 16-byte LDS read), fp32
//                        accumulation, a 32-lane butterfly over the channel chunks, then conv_out's bias and quant_conv
//                        in fp32.
#include <stdlib.h>

#include "common.h"

namespace {

int cu_count() {
    static const int n_cu = [] {
        int dev = 0, n = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return n;
    }();
    return n_cu;
}

// ------------------------------------------------------------------------------------------------ conv_in
template <int DT>
__global__ __launch_bounds__(512) void enc_conv_in_kernel(const float* __restrict__ in, const typename T16<DT>::S* __restrict__ Wk,
                                                         int Kpad, const typename T16<DT>::S* __restrict__ bias,
                                                         typename T16<DT>::S* __restrict__ out, int P, int normalize) {
#pragma clang fp contract(off)
    using S = typename T16<DT>::S;
    using V8 = typename T16<DT>::V8;
    constexpr int CIN = 6, VOX = 512, NROW = 10 * 10 * 10;
    __shared__ __attribute__((aligned(16))) S vol[NROW * 8];         // 16,000 B: rows of (6 channels, 0, 0)

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave = output z-plane
    const int j = lane & 15, q = lane >> 4;

    for (int c = tid; c < NROW; c += 512) reinterpret_cast<u32x4*>(vol)[c] = u32x4{0u, 0u, 0u, 0u};

    // weight fragments: A row j of half ni = cout (j >> 2) * 8 + ni * 4 + (j & 3); k-chunk q of step s = tap 4 s + q
    V8 wf[7][2];
    int toff[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int tap = 4 * s + q;
        toff[s] = tap < 27 ? ((tap / 9 - 1) * 10 + ((tap / 3) % 3 - 1)) * 10 + (tap % 3 - 1) : 0;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int co = (j >> 2) * 8 + ni * 4 + (j & 3);
            V8 v = V8{};
            if (tap < 27) {
#pragma unroll
                for (int e = 0; e < CIN; ++e) v[e] = Wk[(int64_t)co * Kpad + tap * CIN + e];
            }
            wf[s][ni] = v;
        }
    }
    const V8 bv = *reinterpret_cast<const V8*>(bias + q * 8);

    // this thread's voxel (z = w, y, x) and its row in the haloed volume
    const int vy = (tid >> 3) & 7, vx = tid & 7;
    S* myp = vol + ((((w + 1) * 10 + vy + 1) * 10 + vx + 1) << 3);

    float raw[CIN];
    auto load_raw = [&](int p) {
        const float* src = in + (int64_t)p * (CIN * VOX) + tid;
#pragma unroll
        for (int c = 0; c < CIN; ++c) raw[c] = src[c * VOX];
    };
    int p = blockIdx.x;
    if (p < P) load_raw(p);

    // row of this lane's voxel of column group cg for the CENTRE tap: z = w, y = 2 cg + (j >> 3), x = j & 7
    const int row0 = ((w + 1) * 10 + (j >> 3) + 1) * 10 + (j & 7) + 1;

    for (; p < P; p += gridDim.x) {
        __syncthreads();                                             // the previous primitive's fragment reads are done (and the init)
        V8 o = V8{};
#pragma unroll
        for (int c = 0; c < CIN; ++c) {
            float v = raw[c];
            if (normalize) v = c == 0 ? v * 5.0f : v * 2.0f - 1.0f;
            o[c] = (S)v;
        }
        *reinterpret_cast<V8*>(myp) = o;
        if (p + (int)gridDim.x < P) load_raw(p + gridDim.x);
        __syncthreads();

        f32x4 acc[4][2];
#pragma unroll
        for (int cg = 0; cg < 4; ++cg)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[cg][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 7; ++s) {
#pragma unroll
            for (int cg = 0; cg < 4; ++cg) {
                const V8 xf = *reinterpret_cast<const V8*>(vol + ((row0 + cg * 20 + toff[s]) << 3));
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) acc[cg][ni] = T16<DT>::mfma16(wf[s][ni], xf, acc[cg][ni]);
            }
        }

        // lane (j, q) holds voxel w * 64 + cg * 16 + j and channels q * 8 + ni * 4 + r
        const int64_t off0 = ((int64_t)p * VOX + w * 64 + j) * 32 + q * 8;
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) {
            V8 y;
#pragma unroll
            for (int e = 0; e < 8; ++e) y[e] = (S)(acc[cg][e >> 2][e & 3] + (float)bv[e]);
            *reinterpret_cast<V8*>(out + off0 + cg * 16 * 32) = y;
        }
    }
}

// ------------------------------------------------------------------------------------------------ downsample
template <int DT>
__global__ __launch_bounds__(512) void conv3_down_kernel(const typename T16<DT>::S* __restrict__ in,
                                                        const typename T16<DT>::S* __restrict__ Wp,
                                                        const typename T16<DT>::S* __restrict__ bias,
                                                        typename T16<DT>::S* __restrict__ out, int P) {
    using S = typename T16<DT>::S;
    using V8 = typename T16<DT>::V8;
    using V4 = typename T16<DT>::V4;
    constexpr int CIN = 32, VOX = 512, NROW = 10 * 10 * 16, WROWS = 27 * 2 * 16;
    __shared__ __attribute__((aligned(16))) S vol[NROW * 32];        // 102,400 B (the layout of conv3_s8c32_kernel)
    __shared__ __attribute__((aligned(16))) S wl[WROWS * 32];        // 55,296 B

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, q = lane >> 4;
    const int oz = w >> 1, ni = w & 1;                               // output plane, half of the output channels

    for (int c = tid; c < NROW * 4; c += 512) reinterpret_cast<u32x4*>(vol)[c] = u32x4{0u, 0u, 0u, 0u};
    for (int c = tid; c < WROWS * 4; c += 512) reinterpret_cast<u32x4*>(wl)[c] = reinterpret_cast<const u32x4*>(Wp)[c];

    // this thread's INPUT voxel (z = w, y, x) and its row in the haloed volume
    const int vy = (tid >> 3) & 7, vx = tid & 7;
    const int myrow = ((w + 1) * 10 + vy + 1) * 16 + vx + 1;
    S* myp = vol + myrow * 32;
    const int mysw = (myrow >> 1) & 3;

    V8 raw[4];
    auto load_raw = [&](int p) {
        const S* src = in + ((int64_t)p * VOX + tid) * CIN;
#pragma unroll
        for (int c = 0; c < 4; ++c) raw[c] = *reinterpret_cast<const V8*>(src + 8 * c);
    };
    int p = blockIdx.x;
    if (p < P) load_raw(p);

    // row of the CENTRE tap of this lane's output voxel (oz, oy = j >> 2, ox = j & 3): input voxel 2 o
    const int row0 = ((2 * oz + 1) * 10 + 2 * (j >> 2) + 1) * 16 + 2 * (j & 3) + 1;
    const V4 bv = *reinterpret_cast<const V4*>(bias + q * 8 + ni * 4);

    for (; p < P; p += gridDim.x) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) *reinterpret_cast<V8*>(myp + ((c ^ mysw) << 3)) = raw[c];
        if (p + (int)gridDim.x < P) load_raw(p + gridDim.x);
        __syncthreads();

        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 9
        for (int tap = 0; tap < 27; ++tap) {
            const int dz = tap / 9 - 1, dy = (tap / 3) % 3 - 1, dx = tap % 3 - 1;
            const int rw = (tap * 2 + ni) * 16 + j;
            const V8 wfr = *reinterpret_cast<const V8*>(wl + rw * 32 + ((q ^ ((rw >> 1) & 3)) << 3));
            const int r = row0 + (dz * 10 + dy) * 16 + dx;
            const V8 xf = *reinterpret_cast<const V8*>(vol + r * 32 + ((q ^ ((r >> 1) & 3)) << 3));
            acc = T16<DT>::mfma16(wfr, xf, acc);
        }

        // lane (j, q) holds output voxel oz * 16 + j and channels q * 8 + ni * 4 + r
        V4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = (S)(acc[e] + (float)bv[e]);
        *reinterpret_cast<V4*>(out + ((int64_t)p * 64 + oz * 16 + j) * 32 + q * 8 + ni * 4) = y;
    }
}

// ------------------------------------------------------------------------------------------------ head
template <int DT>
__global__ __launch_bounds__(512) void enc_head_kernel(const typename T16<DT>::S* __restrict__ in,
                                                      const typename T16<DT>::S* __restrict__ Wk, int Kpad,
                                                      const float* __restrict__ bias, const float* __restrict__ qw,
                                                      const float* __restrict__ qb, float* __restrict__ out, int P) {
    using S = typename T16<DT>::S;
    using V8 = typename T16<DT>::V8;
    constexpr int C = 256, VOX = 64, K = 27 * C;
    __shared__ __attribute__((aligned(16))) S xs[VOX * C];           // 32,768 B
    __shared__ __attribute__((aligned(16))) S ws[2 * K];             // 27,648 B

    const int tid = threadIdx.x;
    const int c8 = (tid & 31) * 8, row = tid >> 5;                   // 8-channel chunk; row of 4 output voxels (oz, oy)
    const int oz = row >> 2, oy = row & 3;

    for (int c = tid; c < 2 * K / 8; c += 512) {
        const int n = c / (K / 8), k = c - n * (K / 8);
        reinterpret_cast<V8*>(ws)[c] = *reinterpret_cast<const V8*>(Wk + (int64_t)n * Kpad + k * 8);
    }
    const float b0 = bias[0], b1 = bias[1];
    const float q00 = qw[0], q01 = qw[1], q10 = qw[2], q11 = qw[3], qb0 = qb[0], qb1 = qb[1];

    V8 raw[4];
    auto load_raw = [&](int p) {
        const S* src = in + (int64_t)p * (VOX * C) + tid * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) raw[i] = *reinterpret_cast<const V8*>(src + i * 4096);
    };
    int p = blockIdx.x;
    if (p < P) load_raw(p);

    for (; p < P; p += gridDim.x) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<V8*>(xs + tid * 8 + i * 4096) = raw[i];
        if (p + (int)gridDim.x < P) load_raw(p + gridDim.x);
        __syncthreads();

        float acc[4][2];
#pragma unroll
        for (int ox = 0; ox < 4; ++ox) acc[ox][0] = acc[ox][1] = 0.f;
        for (int dz = 0; dz < 3; ++dz) {
            const int iz = oz + dz - 1;
            if (iz < 0 || iz > 3) continue;                          // zero padding: the tap contributes nothing
            for (int dy = 0; dy < 3; ++dy) {
                const int iy = oy + dy - 1;
                if (iy < 0 || iy > 3) continue;
                V8 xv[4];
#pragma unroll
                for (int ix = 0; ix < 4; ++ix) xv[ix] = *reinterpret_cast<const V8*>(xs + ((iz * 4 + iy) * 4 + ix) * C + c8);
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int tap = (dz * 3 + dy) * 3 + dx;
                    const V8 w0 = *reinterpret_cast<const V8*>(ws + tap * C + c8);
                    const V8 w1 = *reinterpret_cast<const V8*>(ws + K + tap * C + c8);
#pragma unroll
                    for (int ox = 0; ox < 4; ++ox) {
                        const int ix = ox + dx - 1;
                        if (ix < 0 || ix > 3) continue;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            acc[ox][0] = __builtin_fmaf((float)xv[ix][e], (float)w0[e], acc[ox][0]);
                            acc[ox][1] = __builtin_fmaf((float)xv[ix][e], (float)w1[e], acc[ox][1]);
                        }
                    }
                }
            }
        }
        // sum over the 32 channel chunks (the 32 lanes of a half wave)
#pragma unroll
        for (int off = 16; off > 0; off >>= 1)
#pragma unroll
            for (int ox = 0; ox < 4; ++ox) {
                acc[ox][0] += __shfl_xor(acc[ox][0], off);
                acc[ox][1] += __shfl_xor(acc[ox][1], off);
            }
        if ((tid & 31) == 0) {
            f32x4 o0, o1;
#pragma unroll
            for (int ox = 0; ox < 4; ++ox) {
                const float y0 = acc[ox][0] + b0, y1 = acc[ox][1] + b1;       // conv_out, fp32 (no rounding to 16 bits)
                o0[ox] = __builtin_fmaf(q01, y1, q00 * y0) + qb0;             // quant_conv (1x1x1, 2 -> 2)
                o1[ox] = __builtin_fmaf(q11, y1, q10 * y0) + qb1;
            }
            float* dst = out + (int64_t)p * (2 * VOX) + row * 4;
            *reinterpret_cast<f32x4*>(dst) = o0;
            *reinterpret_cast<f32x4*>(dst + VOX) = o1;
        }
    }
}

}  // namespace

extern "C" int primx_enc_conv_in(const float* in, const void* Wk, int Kpad, const void* bias, void* out, int P, int normalize,
                                 int dtype, void* stream) {
    PRIMX_REQUIRE(in && Wk && bias && out, "primx_enc_conv_in: null pointer");
    PRIMX_REQUIRE(P > 0 && Kpad >= 162, "primx_enc_conv_in: need P > 0 and Kpad >= 162 (P=%d Kpad=%d)", P, Kpad);
    PRIMX_REQUIRE(((uintptr_t)bias & 15) == 0 && ((uintptr_t)out & 15) == 0, "primx_enc_conv_in: bias and out must be 16-byte aligned");
    const int n_cu = cu_count();
    const dim3 grid(P < 2 * n_cu ? P : 2 * n_cu);
    PRIMX_DISPATCH_16(dtype, "primx_enc_conv_in", {
        using Sx = typename T16<DT>::S;
        hipLaunchKernelGGL((enc_conv_in_kernel<DT>), grid, dim3(512), 0, (hipStream_t)stream, in, (const Sx*)Wk, Kpad, (const Sx*)bias,
                           (Sx*)out, P, normalize);
    });
    PRIMX_CHECK_LAUNCH("primx_enc_conv_in");
    return PRIMX_OK;
}

extern "C" int primx_conv3d_down_s8c32(const void* in, const void* Wp, const void* bias, void* out, int P, int dtype, void* stream) {
    PRIMX_REQUIRE(in && Wp && bias && out, "primx_conv3d_down_s8c32: null pointer");
    PRIMX_REQUIRE(P > 0, "primx_conv3d_down_s8c32: need P > 0 (P=%d)", P);
    PRIMX_REQUIRE((((uintptr_t)in | (uintptr_t)Wp | (uintptr_t)out) & 15) == 0 && ((uintptr_t)bias & 7) == 0,
                  "primx_conv3d_down_s8c32: in, Wp and out must be 16-byte aligned, bias 8-byte aligned");
    const int n_cu = cu_count();
    const dim3 grid(P < n_cu ? P : n_cu);
    PRIMX_DISPATCH_16(dtype, "primx_conv3d_down_s8c32", {
        using Sx = typename T16<DT>::S;
        hipLaunchKernelGGL((conv3_down_kernel<DT>), grid, dim3(512), 0, (hipStream_t)stream, (const Sx*)in, (const Sx*)Wp,
                           (const Sx*)bias, (Sx*)out, P);
    });
    PRIMX_CHECK_LAUNCH("primx_conv3d_down_s8c32");
    return PRIMX_OK;
}

extern "C" int primx_enc_head(const void* in, const void* Wk, int Kpad, const float* bias, const float* qw, const float* qb,
                              float* out, int P, int dtype, void* stream) {
    PRIMX_REQUIRE(in && Wk && bias && qw && qb && out, "primx_enc_head: null pointer");
    PRIMX_REQUIRE(P > 0 && Kpad >= 6912 && Kpad % 8 == 0, "primx_enc_head: need P > 0 and Kpad >= 6912, a multiple of 8 (P=%d Kpad=%d)", P, Kpad);
    PRIMX_REQUIRE((((uintptr_t)in | (uintptr_t)Wk | (uintptr_t)out) & 15) == 0, "primx_enc_head: in, Wk and out must be 16-byte aligned");
    const int n_cu = cu_count();
    const dim3 grid(P < 2 * n_cu ? P : 2 * n_cu);
    PRIMX_DISPATCH_16(dtype, "primx_enc_head", {
        using Sx = typename T16<DT>::S;
        hipLaunchKernelGGL((enc_head_kernel<DT>), grid, dim3(512), 0, (hipStream_t)stream, (const Sx*)in, (const Sx*)Wk, Kpad, bias,
                           qw, qb, out, P);
    });
    PRIMX_CHECK_LAUNCH("primx_enc_head");
    return PRIMX_OK;
}
