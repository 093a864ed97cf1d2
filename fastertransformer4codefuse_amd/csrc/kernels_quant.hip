// Device form of the weight-only int8 quantiser (host_quant.cc quantize_one<T> + host_int8_rowmajor_to_tiled, which follow
// cutlass_preprocessors.cc:576-673): the same arithmetic, operation for operation, so that the tiled bytes and the scale bits are
// what the host function returns for the same values.
//   pass 1  k_quant_colmax : col_max[j] = max_k |float(w[k][j])| (fp32, from 0, `a > max` so a NaN never enters; +-Inf do).  K is
//           cut in 64-row chunks over workgroups; the maximum of non-negative non-NaN floats is the unsigned maximum of their bit
//           patterns, so a workgroup reduces its chunk in registers and LDS and issues one atomicMax per column.
//   pass 2  k_quant_tile   : one 64 (k) x 256 (n) block per workgroup, as the host's 64 x 64 block walk: rows read as whole
//           lines, q = clamp(roundf(float(w) / (col_max / 128))) with the correctly rounded IEEE division (plain `/`; no
//           reciprocal), transposed through padded LDS, every wave stores 1 KiB tiles with one 16-byte store per lane.  The
//           workgroups of the first k tile also store scale[j] = T(col_max[j] / 128).
// Contract: every input whose col_max / 128 is a normal fp32 number or zero (fp16 subnormal inputs and fp16 subnormal scales
// included).  fp32 weights whose column maximum is below about 2^-119 make col_max / 128 an fp32 subnormal: those are outside it.
#include "kernels.h"

namespace ftcf {

namespace {

constexpr int QK_ROWS    = 64;   // rows of a column-maximum chunk (= one k tile)
constexpr int QK_COLS    = 512;  // columns of a column-maximum workgroup: 64 threads x 8
constexpr int QT_COLS    = 256;  // columns of a quantise workgroup: 16 column tiles
constexpr int QT_LDS_DW  = 65;   // LDS row stride in dwords (256 B + 4): the four 16-row lane groups of a tile read 16 banks apart

// eight consecutive elements of a row as fp32 (DT: 0 fp32, 1 fp16, 2 bf16 raw bits)
template<int DT>
__device__ __forceinline__ void load8(const void* base, size_t idx, float (&v)[8])
{
    if constexpr (DT == 0) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + idx);
        const f32x4 b = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + idx + 4);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[i]     = a[i];
            v[4 + i] = b[i];
        }
    }
    else if constexpr (DT == 1) {
        const f16x8 a = *reinterpret_cast<const f16x8*>(reinterpret_cast<const f16*>(base) + idx);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            v[i] = (float)a[i];
        }
    }
    else {
        const u32x4 a = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(base) + idx);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[2 * i]     = __builtin_bit_cast(float, a[i] << 16);
            v[2 * i + 1] = __builtin_bit_cast(float, a[i] & 0xffff0000u);
        }
    }
}

// bf16_t(float) of host_quant.cc: round to nearest even, NaN quieted
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f)
{
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        return ((u >> 16) | 0x40u) & 0xffffu;
    }
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// grid (ceil(N / 512), K / 64, E), 256 threads: thread (tx, ty) owns columns [8 tx, 8 tx + 8) of the strip and rows ty, ty + 4, ...
template<int DT>
__global__ __launch_bounds__(256) void k_quant_colmax(const void* __restrict__ w, size_t K, size_t N, uint32_t* __restrict__ col_max)
{
    __shared__ float red[4][QK_COLS];
    const int        tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const size_t     n0 = (size_t)blockIdx.x * QK_COLS, col = n0 + (size_t)tx * 8;
    const size_t     k0 = (size_t)blockIdx.y * QK_ROWS, e = blockIdx.z;
    float            m[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        m[i] = 0.f;
    }
    if (col < N) {
        const size_t base = (e * K + k0) * N + col;
#pragma unroll 4
        for (int r = ty; r < QK_ROWS; r += 4) {
            float v[8];
            load8<DT>(w, base + (size_t)r * N, v);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const float a = fabsf(v[i]);
                m[i]          = (a > m[i]) ? a : m[i];  // (not fmaxf: a NaN must never become the maximum)
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        red[ty][tx * 8 + i] = m[i];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int    c = h * 256 + (int)threadIdx.x;
        const float  a = red[0][c], b = red[1][c], c2 = red[2][c], d = red[3][c];
        const float  ab = (a > b) ? a : b, cd = (c2 > d) ? c2 : d;
        const float  mx = (ab > cd) ? ab : cd;
        if (n0 + c < N && mx > 0.f) {  // (never a NaN: its bit pattern would sort above Inf)
            atomicMax(col_max + e * N + n0 + c, __builtin_bit_cast(uint32_t, mx));
        }
    }
}

// grid (ceil(N / 256), K / 64, E), 256 threads: thread (g, r0) owns columns [8 g, 8 g + 8) of the block and rows r0, r0 + 8, ...
template<int DT>
__global__ __launch_bounds__(256) void k_quant_tile(const void* __restrict__ w, size_t K, size_t N, const float* __restrict__ col_max,
                                                    uint8_t* __restrict__ out_q, void* __restrict__ out_scale)
{
    __shared__ uint32_t lds[QK_ROWS * QT_LDS_DW];
    const int           g = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const size_t        col = (size_t)blockIdx.x * QT_COLS + (size_t)g * 8;
    const size_t        kt = blockIdx.y, KT = K / TILE_K_I8, NT = N / TILE_N, e = blockIdx.z;
    if (col < N) {
        float cm[8];
        {
            const f32x4 a = *reinterpret_cast<const f32x4*>(col_max + e * N + col);
            const f32x4 b = *reinterpret_cast<const f32x4*>(col_max + e * N + col + 4);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                cm[i]     = a[i] * (1.f / 128.f);  // quant_range_scale = 1 / 2^(bits-1)
                cm[4 + i] = b[i] * (1.f / 128.f);
            }
        }
        if (kt == 0 && r0 == 0) {  // the scale, in the weight dtype
            if constexpr (DT == 0) {
                float* s                            = reinterpret_cast<float*>(out_scale) + e * N + col;
                *reinterpret_cast<f32x4*>(s)        = f32x4{cm[0], cm[1], cm[2], cm[3]};
                *reinterpret_cast<f32x4*>(s + 4)    = f32x4{cm[4], cm[5], cm[6], cm[7]};
            }
            else if constexpr (DT == 1) {
                f16x8 s;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    s[i] = (f16)cm[i];  // round to nearest even, fp16 subnormals kept
                }
                *reinterpret_cast<f16x8*>(reinterpret_cast<f16*>(out_scale) + e * N + col) = s;
            }
            else {
                u32x4 s;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    s[i] = f32_to_bf16_bits(cm[2 * i]) | (f32_to_bf16_bits(cm[2 * i + 1]) << 16);
                }
                *reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(out_scale) + e * N + col) = s;
            }
        }
        const size_t base = (e * K + kt * TILE_K_I8) * N + col;
        float        v[8][8];
#pragma unroll
        for (int p = 0; p < 8; p++) {
            load8<DT>(w, base + (size_t)(r0 + 8 * p) * N, v[p]);
        }
#pragma unroll
        for (int p = 0; p < 8; p++) {
            uint32_t pk[2] = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const float s = roundf(v[p][i] / cm[i]);     // divides by the UNROUNDED fp32 scale; 0 / 0 and Inf / Inf are NaN
                float       c = (s < 127.f) ? s : 127.f;     // std::min(127.f, s): NaN -> 127.f
                if (!(c > -128.f)) {
                    c = (c != c) ? 127.f : -128.f;
                }
                pk[i >> 2] |= (uint32_t)((int)c + 128) << (8 * (i & 3));
            }
            lds[(r0 + 8 * p) * QT_LDS_DW + g * 2]     = pk[0];
            lds[(r0 + 8 * p) * QT_LDS_DW + g * 2 + 1] = pk[1];
        }
    }
    __syncthreads();
    // wave w stores column tiles 4 w .. 4 w + 3 of the block: lane holds q[k = (lane >> 4) * 16 + j][n = lane & 15], j = 0..15
    const int      lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint8_t* lb   = reinterpret_cast<const uint8_t*>(lds);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int    t  = wv * 4 + i;
        const size_t nt = (size_t)blockIdx.x * (QT_COLS / TILE_N) + t;
        if (nt < NT) {
            const uint8_t* src = lb + ((lane >> 4) * 16) * (QT_LDS_DW * 4) + t * 16 + (lane & 15);
            u32x4          o;
#pragma unroll
            for (int j4 = 0; j4 < 4; j4++) {
                uint32_t x = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    x |= (uint32_t)src[(j4 * 4 + j) * (QT_LDS_DW * 4)] << (8 * j);
                }
                o[j4] = x;
            }
            *reinterpret_cast<u32x4*>(out_q + e * K * N + ((nt * KT + kt) * 64 + lane) * 16) = o;
        }
    }
}

template<int DT>
void launch_quant(const void* w, size_t E, size_t K, size_t N, int8_t* out_q, void* out_scale, uint32_t* col_max, hipStream_t s)
{
    const dim3 g1((unsigned)((N + QK_COLS - 1) / QK_COLS), (unsigned)(K / QK_ROWS), (unsigned)E);
    const dim3 g2((unsigned)((N + QT_COLS - 1) / QT_COLS), (unsigned)(K / TILE_K_I8), (unsigned)E);
    hipLaunchKernelGGL(k_quant_colmax<DT>, g1, dim3(256), 0, s, w, K, N, col_max);
    FTCF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_quant_tile<DT>, g2, dim3(256), 0, s, w, K, N, reinterpret_cast<const float*>(col_max),
                       reinterpret_cast<uint8_t*>(out_q), out_scale);
    FTCF_HIP_CHECK(hipGetLastError());
}

}  // namespace

size_t symmetric_quantize_int8_workspace_bytes(size_t E, size_t N)
{
    return E * N * sizeof(float);  // the column maxima
}

void launch_symmetric_quantize_int8(const void* w, int dtype, size_t E, size_t K, size_t N, int8_t* out_q, void* out_scale,
                                    void* workspace, hipStream_t s)
{
    FTCF_CHECK_ARG(K / TILE_K_I8 <= 65535 && E <= 65535, "matrix too large");
    FTCF_HIP_CHECK(hipMemsetAsync(workspace, 0, symmetric_quantize_int8_workspace_bytes(E, N), s));  // the maxima start from 0
    uint32_t* col_max = reinterpret_cast<uint32_t*>(workspace);
    if (dtype == 1) {
        launch_quant<1>(w, E, K, N, out_q, out_scale, col_max, s);
    }
    else if (dtype == 2) {
        launch_quant<2>(w, E, K, N, out_q, out_scale, col_max, s);
    }
    else {
        launch_quant<0>(w, E, K, N, out_q, out_scale, col_max, s);
    }
}

}  // namespace ftcf
