// int16-packed year files (utils/packed.py): each (year file, channel) is stored as 16-bit codes with one fp32 offset and one fp32
// scale, the way GRIB packs a field.  Half the bytes on disk, in the page cache and across PCIe; the fields come back on the device.
//
//   pack     q = clamp(rint((x - offset) / scale), -32767, 32767)      q = -32768 for a non-finite x
//   unpack   xh = (float(q) * scale) + offset                          xh = NaN for q = -32768
//
// Every step is ONE fp32 operation that numpy reproduces bit for bit: no fused multiply-add may be formed from the product and the
// sum of the unpack.  The `fp contract(off)` pragma below forbids it for every operation written in this file, and the operations are
// written with the plain operators for that reason: this compiler's headers define __fmul_rn / __fadd_rn / __fsub_rn as the plain
// operators too, but up there, under the default contraction, and the unpack written with them came out as v_pk_fma_f32 even with the
// pragma in place.  With the operators the disassembly shows v_pk_mul_f32 + v_pk_add_f32.  The division is the IEEE division
// era5_select_normalize_kernel (dataio.hip) relies on, rintf rounds half to even.  utils/packed.py states the rule in numpy;
// tests/packed_reference.py restates it and derives the error bound.
//
//   era5_select_normalize_i16_kernel<V>  the training path: dataio.hip's crop + channel select + z-score with the unpack in front.
//                                        Reads 2 B, writes 4 B per element.  A lane takes V = 8 codes (one 16-byte load, two 16-byte
//                                        stores) where every row start is 16-byte aligned (Wraw % 8 == 0, W % 8 == 0), else V = 4 codes
//                                        (one 8-byte load, one 16-byte store): with Wraw % 8 == 4 every other row is only 8-byte aligned.
//   era5_unpack_i16_kernel<V>            a whole slab [C][H][W] back to fp32 with one parameter row (statistics, unpacking a folder)
//   era5_pack_i16_kernel<V>              the pack rule over a slab
//   pack_range_kernel / _fold_kernel     per-channel minimum / maximum of the finite values and the number of the others: the slice plan
//                                        of plane_stream.h with planes = C, workgroup (c, slice) owns ws[c][slice]; one wave per channel
//                                        folds the slices into the running range / missing of the year file.  Minima, maxima and integer
//                                        counts do not depend on the order, so two runs agree bit for bit.
#include <math.h>

#include <type_traits>

#include "plane_stream.h"

#pragma clang fp contract(off)

typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int PACK_MISSING = -32768;            // the code of a non-finite value
constexpr float PACK_QMAX = 32767.0f;

struct PackRangePart {                          // ws[c][slice] of swv2_pack_range: 16 bytes
    float lo, hi;
    long long missing;
};

__device__ __forceinline__ bool pack_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ float unpack_one(int q, float scale, float offset) {
    const float v = ((float)q * scale) + offset;            // two roundings
    return q == PACK_MISSING ? __uint_as_float(0x7fc00000u) : v;
}

__device__ __forceinline__ short pack_one(float x, float scale, float offset) {
    float r = rintf((x - offset) / scale);
    r = fminf(fmaxf(r, -PACK_QMAX), PACK_QMAX);
    return (short)(pack_finite(x) ? (int)r : PACK_MISSING);
}

// V codes at p (V * 2 bytes, aligned to that) -> V / 4 vectors of four floats
template <int V>
__device__ __forceinline__ void unpack_vec(const short* __restrict__ p, float scale, float offset, f32x4 (&v)[V / 4]) {
    if constexpr (V == 8) {
        const i16x8 q = *(const i16x8*)p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e / 4][e % 4] = unpack_one(q[e], scale, offset);
    } else {
        const i16x4 q = *(const i16x4*)p;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[0][e] = unpack_one(q[e], scale, offset);
    }
}

// out[b][coff + s*Csel + c][i][j] = (xh - mean[c]) / std[c],  xh = unpack(raw[b][s][chan[c]][i][j]) with the parameters of row
// slab_row[b*S + s] of the offset / scale tables [rows][Craw]      (i < H, j < W)
template <int V>
__global__ __launch_bounds__(256) void era5_select_normalize_i16_kernel(
    const short* __restrict__ raw, float* __restrict__ out, const int* __restrict__ chan, const float* __restrict__ mean,
    const float* __restrict__ stdv, const float* __restrict__ offset, const float* __restrict__ scale, const int* __restrict__ slab_row,
    int S, int Csel, int Craw, int Hraw, int Wraw, int H, int W, int Cout_total, int coff) {
    const int plane = blockIdx.y;                          // (b, s, c)
    const int c = plane % Csel, s = (plane / Csel) % S, b = plane / (Csel * S);
    const float m = mean[c], sd = stdv[c];
    const int ch = chan[c];
    const size_t prm = (size_t)slab_row[b * S + s] * Craw + ch;
    const float sc = scale[prm], off = offset[prm];
    const short* src = raw + (((size_t)b * S + s) * Craw + ch) * (size_t)Hraw * Wraw;
    float* dst = out + ((size_t)b * Cout_total + coff + s * Csel + c) * (size_t)H * W;
    const int Wv = W / V;                                  // W % V == 0 and Wraw % V == 0 (the host picks V)
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < H * Wv; idx += gridDim.x * blockDim.x) {
        const int i = idx / Wv, jv = idx - i * Wv;
        f32x4 v[V / 4];
        unpack_vec<V>(src + (size_t)i * Wraw + V * jv, sc, off, v);
#pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[k][e] - m) / sd;      // dataio.hip's z-score, bit for bit
            *(f32x4*)(dst + (size_t)i * W + V * jv + 4 * k) = o;
        }
    }
}

// out[c][e] = unpack(raw[c][e]) with offset[c], scale[c]      (e < plane = H * W, a multiple of V)
template <int V>
__global__ __launch_bounds__(256) void era5_unpack_i16_kernel(const short* __restrict__ raw, float* __restrict__ out,
                                                              const float* __restrict__ offset, const float* __restrict__ scale, uint32_t plane) {
    const int c = blockIdx.y;
    const float sc = scale[c], off = offset[c];
    const short* src = raw + (size_t)c * plane;
    float* dst = out + (size_t)c * plane;
    const uint32_t nv = plane / V;
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nv; idx += gridDim.x * blockDim.x) {
        f32x4 v[V / 4];
        unpack_vec<V>(src + (size_t)idx * V, sc, off, v);
#pragma unroll
        for (int k = 0; k < V / 4; ++k) *(f32x4*)(dst + (size_t)idx * V + 4 * k) = v[k];
    }
}

// out[c][e] = pack(slab[c][e]) with offset[c], scale[c]
template <int V>
__global__ __launch_bounds__(256) void era5_pack_i16_kernel(const float* __restrict__ slab, short* __restrict__ out,
                                                            const float* __restrict__ offset, const float* __restrict__ scale, uint32_t plane) {
    const int c = blockIdx.y;
    const float sc = scale[c], off = offset[c];
    const float* src = slab + (size_t)c * plane;
    short* dst = out + (size_t)c * plane;
    const uint32_t nv = plane / V;
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nv; idx += gridDim.x * blockDim.x) {
        typename std::conditional<V == 8, i16x8, i16x4>::type q;
#pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            const f32x4 x = *(const f32x4*)(src + (size_t)idx * V + 4 * k);
#pragma unroll
            for (int e = 0; e < 4; ++e) q[4 * k + e] = pack_one(x[e], sc, off);
        }
        *(decltype(q)*)(dst + (size_t)idx * V) = q;
    }
}

// Workgroup (c, slice): minimum and maximum of the finite values of its slice, the number of the others.
__global__ __launch_bounds__(256) void pack_range_kernel(const float* __restrict__ slab, PackRangePart* __restrict__ ws, int H, int W, int slices) {
    const int c = blockIdx.x / slices, sl = blockIdx.x - c * slices;
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30, a multiple of 4 (checked by the host)
    uint32_t lo, hi;
    plane_slice_range(plane, sl, slices, lo, hi);
    const float* x = slab + (size_t)c * plane;
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (uint32_t i = lo + threadIdx.x * 4; i < hi; i += 1024) {
        const f32x4 v = *(const f32x4*)(x + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool f = pack_finite(v[e]);
            mn = fminf(mn, f ? v[e] : INFINITY);
            mx = fmaxf(mx, f ? v[e] : -INFINITY);
            bad += f ? 0 : 1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
        bad += __shfl_xor(bad, o);
    }
    __shared__ float rmn[4], rmx[4];
    __shared__ int rbad[4];
    if ((threadIdx.x & 63) == 0) {
        rmn[threadIdx.x >> 6] = mn;
        rmx[threadIdx.x >> 6] = mx;
        rbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                   // the one owner of ws[c][sl]; an empty slice stores (+inf, -inf, 0)
        PackRangePart p;
        p.lo = fminf(fminf(rmn[0], rmn[1]), fminf(rmn[2], rmn[3]));
        p.hi = fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3]));
        p.missing = (long long)rbad[0] + rbad[1] + rbad[2] + rbad[3];
        ws[blockIdx.x] = p;
    }
}

// One wave per channel: the slices of the slab into the year file's running range [C][2] and missing [C].
__global__ __launch_bounds__(64) void pack_range_fold_kernel(const PackRangePart* __restrict__ ws, int slices, float* __restrict__ range,
                                                             long long* __restrict__ missing, int first) {
    const int c = blockIdx.x, lane = threadIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    long long bad = 0;
    for (int sl = lane; sl < slices; sl += 64) {
        const PackRangePart p = ws[(size_t)c * slices + sl];
        mn = fminf(mn, p.lo);
        mx = fmaxf(mx, p.hi);
        bad += p.missing;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
        bad += __shfl_xor(bad, o);
    }
    if (lane == 0) {
        if (!first) {
            mn = fminf(mn, range[2 * c]);
            mx = fmaxf(mx, range[2 * c + 1]);
            bad += missing[c];
        }
        range[2 * c] = mn;
        range[2 * c + 1] = mx;
        missing[c] = bad;
    }
}

// a slab [C][H][W]: the grid of the per-element kernels, V elements per lane, four vectors per thread
inline dim3 slab_grid(int C, long plane, int V) { return dim3(cdiv(plane / V, 256 * 4), C); }

}  // namespace

extern "C" int swv2_era5_select_normalize_i16(const int16_t* raw, float* out, const int* chan, const float* mean, const float* stdv,
                                              const float* offset, const float* scale, const int* slab_row, int B, int S, int Csel, int Craw,
                                              int Hraw, int Wraw, int H, int W, int Cout_total, int coff, void* stream) {
    SWV2_CHECK_ARG(raw && out && chan && mean && stdv && offset && scale && slab_row, "swv2_era5_select_normalize_i16: null pointer");
    SWV2_CHECK_ARG(B > 0 && S > 0 && Csel > 0 && Craw > 0 && H > 0 && H <= Hraw && W > 0 && W <= Wraw,
                   "swv2_era5_select_normalize_i16: bad sizes");
    SWV2_CHECK_ARG(W % 4 == 0 && Wraw % 4 == 0, "swv2_era5_select_normalize_i16: W=%d, Wraw=%d must be multiples of 4", W, Wraw);
    SWV2_CHECK_ARG(((uintptr_t)raw & 7) == 0, "swv2_era5_select_normalize_i16: raw not 8-byte aligned");
    SWV2_CHECK_ARG(((uintptr_t)out & 15) == 0, "swv2_era5_select_normalize_i16: out not 16-byte aligned");
    SWV2_CHECK_ARG(coff >= 0 && coff + (long)S * Csel <= Cout_total, "swv2_era5_select_normalize_i16: channel range outside the output");
    SWV2_CHECK_ARG((long)B * S * Csel <= 65535, "swv2_era5_select_normalize_i16: B * S * Csel = %ld planes exceed the grid's 65535",
                   (long)B * S * Csel);
    const bool v8 = W % 8 == 0 && Wraw % 8 == 0 && ((uintptr_t)raw & 15) == 0;      // every row start 16-byte aligned
    dim3 grid(cdiv((long)H * (W / (v8 ? 8 : 4)), 256 * 4), B * S * Csel);
    if (v8)
        hipLaunchKernelGGL(era5_select_normalize_i16_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, raw, out, chan, mean, stdv, offset,
                           scale, slab_row, S, Csel, Craw, Hraw, Wraw, H, W, Cout_total, coff);
    else
        hipLaunchKernelGGL(era5_select_normalize_i16_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, raw, out, chan, mean, stdv, offset,
                           scale, slab_row, S, Csel, Craw, Hraw, Wraw, H, W, Cout_total, coff);
    SWV2_CHECK_LAUNCH("swv2_era5_select_normalize_i16");
    return SWV2_OK;
}

// what swv2_era5_unpack_i16 and swv2_era5_pack_i16 share: slab [C][H][W] with planes of a multiple of 4 elements
static int slab_args_ok(const char* who, const void* i16, const void* f32, const void* offset, const void* scale, int C, int H, int W) {
    if (!(i16 && f32 && offset && scale)) return swv2_set_error("%s: null pointer", who), 0;
    if (!(C > 0 && C <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 30)))
        return swv2_set_error("%s: bad sizes (C in 1 .. 65535, H, W > 0, H * W < 2^30)", who), 0;
    if (W % 4 != 0) return swv2_set_error("%s: W %% 4 != 0 (W=%d)", who, W), 0;
    if ((uintptr_t)i16 & 7) return swv2_set_error("%s: int16 pointer not 8-byte aligned", who), 0;
    if ((uintptr_t)f32 & 15) return swv2_set_error("%s: fp32 pointer not 16-byte aligned", who), 0;
    return 1;
}

extern "C" int swv2_era5_unpack_i16(const int16_t* raw, float* out, const float* offset, const float* scale, int C, int H, int W, void* stream) {
    if (!slab_args_ok("swv2_era5_unpack_i16", raw, out, offset, scale, C, H, W)) return SWV2_ERR_INVALID;
    const long plane = (long)H * W;
    if (plane % 8 == 0 && ((uintptr_t)raw & 15) == 0)
        hipLaunchKernelGGL(era5_unpack_i16_kernel<8>, slab_grid(C, plane, 8), dim3(256), 0, (hipStream_t)stream, raw, out, offset, scale,
                           (uint32_t)plane);
    else
        hipLaunchKernelGGL(era5_unpack_i16_kernel<4>, slab_grid(C, plane, 4), dim3(256), 0, (hipStream_t)stream, raw, out, offset, scale,
                           (uint32_t)plane);
    SWV2_CHECK_LAUNCH("swv2_era5_unpack_i16");
    return SWV2_OK;
}

extern "C" int swv2_era5_pack_i16(const float* slab, int16_t* out, const float* offset, const float* scale, int C, int H, int W, void* stream) {
    if (!slab_args_ok("swv2_era5_pack_i16", out, slab, offset, scale, C, H, W)) return SWV2_ERR_INVALID;
    const long plane = (long)H * W;
    if (plane % 8 == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(era5_pack_i16_kernel<8>, slab_grid(C, plane, 8), dim3(256), 0, (hipStream_t)stream, slab, out, offset, scale,
                           (uint32_t)plane);
    else
        hipLaunchKernelGGL(era5_pack_i16_kernel<4>, slab_grid(C, plane, 4), dim3(256), 0, (hipStream_t)stream, slab, out, offset, scale,
                           (uint32_t)plane);
    SWV2_CHECK_LAUNCH("swv2_era5_pack_i16");
    return SWV2_OK;
}

extern "C" size_t swv2_pack_range_ws_bytes(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)C * plane_slices(C) * sizeof(PackRangePart);
}

extern "C" int swv2_pack_range(const float* slab, int C, int H, int W, int first, float* range, int64_t* missing, void* ws, size_t ws_bytes,
                               void* stream) {
    SWV2_CHECK_ARG(slab && range && missing && ws, "swv2_pack_range: null pointer");
    SWV2_CHECK_ARG(plane_shape_ok(C, H, W), "swv2_pack_range: bad shape (C, H, W > 0, C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG(W % 4 == 0, "swv2_pack_range: W %% 4 != 0 (W=%d)", W);
    SWV2_CHECK_ARG((((uintptr_t)missing | (uintptr_t)ws) & 7) == 0 && ((uintptr_t)range & 3) == 0,
                   "swv2_pack_range: pointer not aligned (missing, ws: 8 bytes; range: 4)");
    if (!plane_operands_ok("swv2_pack_range", {slab}, {}, 1, 0, ws_bytes, swv2_pack_range_ws_bytes(C, H, W), "swv2_pack_range_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices(C);
    hipLaunchKernelGGL(pack_range_kernel, dim3((unsigned)((long)C * slices)), dim3(256), 0, (hipStream_t)stream, slab, (PackRangePart*)ws, H, W,
                       slices);
    SWV2_CHECK_LAUNCH("swv2_pack_range");
    hipLaunchKernelGGL(pack_range_fold_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, (const PackRangePart*)ws, slices, range, (long long*)missing, first);
    SWV2_CHECK_LAUNCH("swv2_pack_range (fold)");
    return SWV2_OK;
}
