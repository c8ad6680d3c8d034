// cnn_kernels.hip -- the convolution trunk of the crowd sensor's policy (AMPSeptCNNBuilder `_task_actor_cnn`), one launch.
//
// What the reference does per policy step (amp_network_sept_cnn_builder.py:49-67 over network_builder.py:125-148): view the map
// columns of the normalised observation as (B, res, res, C), permute to NCHW, run up to four Conv2d(kernel 4, stride 2, padding 1)
// + ReLU, flatten in (channel, row, column) order.  Here one workgroup of 256 lanes runs that whole tower for one env: it reads the RAW
// map columns of the observation row, applies RunningMeanStd's normalisation and clamp as it loads (the arithmetic and the operation
// order of obs_normalize_kernel, predictor_kernels.hip), keeps every activation in LDS and writes only the flattened features.
//
// Layout.  Every LDS image is [channel][row + 1][column + 1] with one zero column on either side and zero rows where the convolution's
// padding falls, so the inner loop has no bounds test, and a lane's four kernel columns start at the even column 2 * ox: two 8-byte
// reads, lane stride 8 bytes.  The first layer is produced in bands: the second layer's rows are taken kCnnBand at a time, the band
// needs 2 * kCnnBand + 2 rows of the first layer (two of them carried over from the band before), and those need 4 * kCnnBand + 4
// rows of the input, staged (normalised) just before.  Neither the 48 KB input nor the 64 KB first-layer output of the 64 x 64 x 3
// shape ever sits in LDS whole: 3 960 + 5 440 + 5 184 + 1 600 floats = 64 736 bytes, two workgroups per CU.
//
// Work split.  Wave w of the four owns filters [4w, 4w + 4) of every layer; its lanes own output pixels (row-major, 64 at a time) and
// keep four accumulators.  The filter index is wave-uniform, so the weights come through the scalar (constant) path; an input value
// read from LDS feeds four fused multiply-adds.
//
// Arithmetic.  fp32, one fixed order per output value:  acc = bias[f];  for ci, for ky, for kx:  acc = fmaf(in, w[f][ci][ky][kx], acc);
// out = fmaxf(acc, 0).  Padding positions take part as fmaf(0, w, acc).  The unit is built with -ffp-contract=off, so the CPU
// emulation (tests/emu/emu_cnn.cpp, the same source) gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace emloco {

constexpr int kCnnThreads = 256;
constexpr int kCnnMaxRes = 64, kCnnMaxFilters = 16, kCnnMaxLayers = 4, kCnnMaxChannels = 3;
constexpr int kCnnBand = 4;                                  // rows of the second layer per band
constexpr int kCnnL1Slots = 2 * kCnnBand + 2;                // rows of the first layer a band reads
constexpr int kCnnL1New = 2 * kCnnBand + 1;                  // rows of the first layer a band computes at most (the first band)
constexpr int kCnnInSlots = 2 * kCnnL1New + 2;               // rows of the input those read
constexpr int kCnnInFloats = kCnnMaxChannels * kCnnInSlots * (kCnnMaxRes + 2);
constexpr int kCnnL1Floats = kCnnMaxFilters * kCnnL1Slots * (kCnnMaxRes / 2 + 2);
constexpr int kCnnL2Floats = kCnnMaxFilters * (kCnnMaxRes / 4 + 2) * (kCnnMaxRes / 4 + 2);
constexpr int kCnnL3Floats = kCnnMaxFilters * (kCnnMaxRes / 8 + 2) * (kCnnMaxRes / 8 + 2);

struct CnnTrunk {
    int rows, res, channels, layers;
    int filters[kCnnMaxLayers];
    int ldx, ldo, out_off, normalize;
    float eps, clip;
    const float *x, *mean, *var, *params;
    float *out;
};

// why the arguments cannot be served, or nullptr; the text names the argument (cnn_capi.hip and the emulator share it)
inline const char *cnn_refusal(const CnnTrunk &a) {
    if (!a.x) return "x is null";
    if (!a.params) return "params is null";
    if (!a.out) return "out is null";
    if (a.normalize && !a.mean) return "mean is null";
    if (a.normalize && !a.var) return "var is null";
    if (a.rows < 1) return "rows must be at least 1";
    if (a.res < 8 || a.res > kCnnMaxRes || a.res % 8) return "res must be a multiple of 8, at most 64";
    if (a.channels != 1 && a.channels != 3) return "channels must be 1 or 3";
    if (a.layers < 1 || a.layers > kCnnMaxLayers) return "layers must be 1 to 4";
    if (a.res % (1 << a.layers)) return "res does not halve cleanly through every one of the layers";
    for (int l = 0; l < a.layers; ++l)
        if (a.filters[l] < 1 || a.filters[l] > kCnnMaxFilters) return "filters must be 1 to 16 in every layer";
    if (a.ldx < a.channels * a.res * a.res) return "ldx is smaller than the map's width";
    const int side = a.res >> a.layers;
    if (a.out_off < 0) return "out_off is negative";
    if (a.ldo < a.out_off + a.filters[a.layers - 1] * side * side) return "ldo is smaller than out_off plus the feature width";
    return nullptr;
}

struct alignas(8) cnn_f2 { float x, y; };

// Rows [0, n_rows) x columns [0, w_out) of one layer's output for this wave's four filters.  `in`: padded LDS image, `in_slot` the
// row slot that holds input row 2 * (first output row) - 1.  Output value (f, oy, ox) goes to out[f * o_plane + oy * o_row + ox + o_base].
__device__ __forceinline__ void cnn_conv(const float *in, int cin, int in_plane, int in_wp, int in_slot, const float *__restrict__ w,
                                         const float *__restrict__ bias, int nf, int wave, int n_rows, int w_out, float *out, int o_plane,
                                         int o_row, int o_base) {
    const int f0 = wave * 4;
    if (f0 >= nf) return;                                   // (wave-uniform; the barriers are the caller's)
    const int lane = (int)(threadIdx.x & 63u);
    int fi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) fi[q] = f0 + q < nf ? f0 + q : nf - 1;        // a short last group repeats its last filter and does not store it
    const int npix = n_rows * w_out;
    for (int p = lane; p < npix; p += 64) {
        const int oy = p / w_out, ox = p - oy * w_out;
        float acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = bias[fi[q]];
        const float *src = in + (in_slot + 2 * oy) * in_wp + 2 * ox;
        for (int ci = 0; ci < cin; ++ci) {
            const float *s = src + ci * in_plane;
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const cnn_f2 lo = *reinterpret_cast<const cnn_f2 *>(s + ky * in_wp);
                const cnn_f2 hi = *reinterpret_cast<const cnn_f2 *>(s + ky * in_wp + 2);
                const float v[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
                for (int kx = 0; kx < 4; ++kx)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = fmaf(v[kx], w[(fi[q] * cin + ci) * 16 + ky * 4 + kx], acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (f0 + q < nf) out[(f0 + q) * o_plane + oy * o_row + ox + o_base] = fmaxf(acc[q], 0.0f);
    }
}

// (the pointers travel beside the struct: `const ... __restrict__` kernel arguments are what lets the wave-uniform weight reads take the
// scalar path)
__global__ void __launch_bounds__(kCnnThreads)
cnn_trunk_kernel(const CnnTrunk a, const float *__restrict__ xin, const float *__restrict__ mean, const float *__restrict__ var,
                 const float *__restrict__ params, float *__restrict__ outp) {
    __shared__ __attribute__((aligned(16))) float s_in[kCnnInFloats];
    __shared__ __attribute__((aligned(16))) float s_l1[kCnnL1Floats];
    __shared__ __attribute__((aligned(16))) float s_l2[kCnnL2Floats];
    __shared__ __attribute__((aligned(16))) float s_l3[kCnnL3Floats];
    const int tid = (int)threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int H0 = a.res, H1 = H0 >> 1, H2 = H0 >> 2, H3 = H0 >> 3, H4 = H0 >> 4;
    const int C0 = a.channels, F1 = a.filters[0], F2 = a.filters[1], F3 = a.filters[2], F4 = a.filters[3];
    // params: for every layer its weights [F][Cin][4][4], then its bias [F]
    const float *w1 = params, *b1 = w1 + F1 * C0 * 16;
    const float *w2 = b1 + F1, *b2 = w2 + F2 * F1 * 16;
    const float *w3 = b2 + F2, *b3 = w3 + F3 * F2 * 16;
    const float *w4 = b3 + F3, *b4 = w4 + F4 * F3 * 16;
    const int in_wp = H0 + 2, in_plane = kCnnInSlots * in_wp;
    const int l1_wp = H1 + 2, l1_plane = kCnnL1Slots * l1_wp;
    const int l2_wp = H2 + 2, l2_plane = (H2 + 2) * l2_wp;
    const int l3_wp = H3 + 2, l3_plane = (H3 + 2) * l3_wp;
    const int row_floats = H0 * C0;

    // the zero columns and the zero rows above and below the whole images are written here and never again
    for (int i = tid; i < kCnnInFloats; i += kCnnThreads) s_in[i] = 0.0f;
    for (int i = tid; i < kCnnL1Floats; i += kCnnThreads) s_l1[i] = 0.0f;
    for (int i = tid; i < kCnnL2Floats; i += kCnnThreads) s_l2[i] = 0.0f;
    for (int i = tid; i < kCnnL3Floats; i += kCnnThreads) s_l3[i] = 0.0f;
    __syncthreads();

    for (long row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const float *x = xin + row * a.ldx;
        float *out = outp + row * a.ldo + a.out_off;

        // input rows [2 la - 1, 2 lb + 1), normalised, into slots 0.. of s_in (what first-layer rows [la, lb) read); rows outside the map are zero
        auto stage_input = [&](int la, int lb) {
            const int y0 = 2 * la - 1, total = (2 * (lb - la) + 2) * row_floats;
            for (int i = tid; i < total; i += kCnnThreads) {
                const int r = i / row_floats, rem = i - r * row_floats;
                const int xc = rem / C0, c = rem - xc * C0, y = y0 + r;
                float v = 0.0f;
                if (y >= 0 && y < H0) {
                    const int g = y * row_floats + rem;
                    v = x[g];
                    if (a.normalize) {
                        v = (v - mean[g]) / sqrtf(var[g] + a.eps);
                        v = fminf(fmaxf(v, -a.clip), a.clip);
                    }
                }
                s_in[c * in_plane + r * in_wp + xc + 1] = v;
            }
        };

        if (a.layers == 1) {
            for (int la = 0; la < H1; la += 2 * kCnnBand) {
                const int lb = la + 2 * kCnnBand < H1 ? la + 2 * kCnnBand : H1;
                stage_input(la, lb);
                __syncthreads();
                cnn_conv(s_in, C0, in_plane, in_wp, 0, w1, b1, F1, wave, lb - la, H1, out, H1 * H1, H1, la * H1);
                __syncthreads();
            }
            continue;
        }

        // bands of the second layer: rows [r0, r1) read first-layer rows 2 r0 - 1 .. 2 r1, slot j of s_l1 holding row 2 r0 - 1 + j
        for (int r0 = 0; r0 < H2; r0 += kCnnBand) {
            const int r1 = r0 + kCnnBand < H2 ? r0 + kCnnBand : H2;
            const int la = r0 == 0 ? 0 : 2 * r0 + 1;                      // (rows 2 r0 - 1 and 2 r0 were carried over)
            const int lb = 2 * r1 + 1 < H1 ? 2 * r1 + 1 : H1;
            stage_input(la, lb);
            if (r0 == 0)                                                  // row -1: padding
                for (int i = tid; i < F1 * H1; i += kCnnThreads) s_l1[(i / H1) * l1_plane + (i % H1) + 1] = 0.0f;
            if (2 * r1 == H1)                                             // row H1: padding
                for (int i = tid; i < F1 * H1; i += kCnnThreads) s_l1[(i / H1) * l1_plane + (H1 - (2 * r0 - 1)) * l1_wp + (i % H1) + 1] = 0.0f;
            __syncthreads();
            cnn_conv(s_in, C0, in_plane, in_wp, 0, w1, b1, F1, wave, lb - la, H1, s_l1, l1_plane, l1_wp, (la - (2 * r0 - 1)) * l1_wp + 1);
            __syncthreads();
            if (a.layers == 2)
                cnn_conv(s_l1, F1, l1_plane, l1_wp, 0, w2, b2, F2, wave, r1 - r0, H2, out, H2 * H2, H2, r0 * H2);
            else
                cnn_conv(s_l1, F1, l1_plane, l1_wp, 0, w2, b2, F2, wave, r1 - r0, H2, s_l2, l2_plane, l2_wp, (r0 + 1) * l2_wp + 1);
            __syncthreads();
            if (r1 < H2) {                                                // the next band's rows 2 r1 - 1 and 2 r1: slots 2 kCnnBand, + 1 -> 0, 1
                for (int i = tid; i < F1 * 2 * H1; i += kCnnThreads) {
                    const int f = i / (2 * H1), rem = i - f * 2 * H1, j = rem / H1, c = rem - j * H1;
                    s_l1[f * l1_plane + j * l1_wp + c + 1] = s_l1[f * l1_plane + (2 * kCnnBand + j) * l1_wp + c + 1];
                }
                __syncthreads();
            }
        }
        if (a.layers >= 3) {
            if (a.layers == 3)
                cnn_conv(s_l2, F2, l2_plane, l2_wp, 0, w3, b3, F3, wave, H3, H3, out, H3 * H3, H3, 0);
            else
                cnn_conv(s_l2, F2, l2_plane, l2_wp, 0, w3, b3, F3, wave, H3, H3, s_l3, l3_plane, l3_wp, l3_wp + 1);
            __syncthreads();
        }
        if (a.layers == 4) {
            cnn_conv(s_l3, F3, l3_plane, l3_wp, 0, w4, b4, F4, wave, H4, H4, out, H4 * H4, H4, 0);
            __syncthreads();
        }
    }
}

}  // namespace emloco
