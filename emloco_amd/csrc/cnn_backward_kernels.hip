// cnn_backward_kernels.hip -- the weight and bias gradients of the convolution trunk (cnn_kernels.hip), two launches, nothing saved
// between forward and backward.
//
// What the reference gets from autograd over amp_network_sept_cnn_builder.py:49-67: d loss / d (every Conv2d weight and bias of
// `_task_actor_cnn`), summed over the batch.  Here one workgroup of 512 lanes takes one row at a time: it recomputes every activation
// from x and params with cnn_conv (the forward's arithmetic, bit for bit, so the ReLU masks are the forward's), keeps them in LDS, and
// walks back down.  Neither the normalised map nor an activation nor an activation gradient goes to HBM.  No gradient with respect to
// the map is produced: the observations are data.
//
// Per row, `layers` >= 2:
//   sweep 1   the forward's bands; layers 2, 3 and 4 are kept whole (padded images, zero border).
//   top       dtop = dout . [top > 0] into the top layer's padded gradient image.
//   k = layers .. 3:  dW_k / db_k from d_k (*) L_(k-1);  d_(k-1) = gather(d_k, W_k) . [L_(k-1) > 0].
//   sweep 2   the bands again: the input band is re-staged and the first-layer band recomputed (carried-over rows as in the forward);
//             dW_2 / db_2 from d_2's rows of the band (*) the first-layer slots; d_1 for the band's NEW first-layer rows in gather form
//             from the whole d_2 (no band-edge hand-over); dW_1 / db_1 from d_1 (*) the staged input.
// `layers` == 1: one sweep, d_1 = dout . [L_1 > 0] band by band.
//
// Gather form of the data gradient (Conv2d k 4, s 2, p 1): pixel (ci, y, x) of the layer below receives, from every filter f, the four
// taps ky in {(y + 1) & 1, + 2}, kx likewise, of output pixel ((y + 1 - ky) / 2, (x + 1 - kx) / 2); the zero border of the padded
// gradient image serves the output pixels that do not exist.  The weights are read per lane here (two addresses per wave and tap).
//
// Weight gradients, deterministic, no float atomics.  For layer k lane t owns the pair (f, ci) = t mod (F_k * Cin_k) -- sixteen
// accumulators, one per kernel tap, and the bias's -- and the pixel share t / (F_k * Cin_k) of 512 / (F_k * Cin_k): it visits the
// pixels p = share, share + shares, ... of every phase in ascending order, row after row of the rows its workgroup strides through, and
// keeps the sums in registers until the kernel's end.  Layers 1 and 2 split over all 512 lanes; layers 3 and 4, a few pixels each, take
// one half of the workgroup each and share one accumulator set (a fourth set costs 136-164 bytes of scratch at the 256-register cap
// of two waves per SIMD).  Then the shares are summed through LDS in ascending order and the workgroup
// writes its partial [P] vector to workspace[block][P]; cnn_grad_reduce_kernel sums the partials over blocks in ascending order.  The
// grid is cnn_bwd_grid(rows), a pure function of rows, so the same inputs give the same bits on every run and on the CPU emulation
// (tests/emu/emu_cnn_bwd.cpp, the same source; the unit is built with -ffp-contract=off).
//
// LDS: 28 600 floats = 114 400 bytes (static), one workgroup per CU, hence 512 lanes (two waves per SIMD).  In the recomputation waves
// 4-7 take the lower half of a phase's rows with the filters of waves 0-3.
#pragma once
#include "cnn_kernels.hip"

namespace emloco {

constexpr int kCnnBwdThreads = 512;
constexpr int kCnnBwdMaxGrid = 256;                          // one workgroup per CU of an MI355X
constexpr int kCnnD1Plane = kCnnL1New * (kCnnMaxRes / 2);    // the band's first-layer gradient, unpadded [f][row][column]
constexpr int kCnnL4Floats = kCnnMaxFilters * (kCnnMaxRes / 16 + 2) * (kCnnMaxRes / 16 + 2);
// offsets into the one LDS array
constexpr int kBwdIn = 0, kBwdL1 = kBwdIn + kCnnInFloats, kBwdL2 = kBwdL1 + kCnnL1Floats, kBwdL3 = kBwdL2 + kCnnL2Floats,
              kBwdL4 = kBwdL3 + kCnnL3Floats, kBwdD1 = kBwdL4 + kCnnL4Floats, kBwdD2 = kBwdD1 + kCnnMaxFilters * kCnnD1Plane,
              kBwdD3 = kBwdD2 + kCnnL2Floats, kBwdD4 = kBwdD3 + kCnnL3Floats, kBwdLdsFloats = kBwdD4 + kCnnL4Floats;
static_assert(kBwdLdsFloats * 4 <= 160 * 1024, "the backward's LDS plan must fit a gfx950 CU");
static_assert(kBwdLdsFloats >= kCnnBwdThreads * 17, "the share reduction reuses the images");

struct CnnTrunkBwd {
    CnnTrunk t;                       // the forward's operands; t.out / t.ldo / t.out_off are not used
    const float *dout;
    int lddo, dout_off;
    float *dparams, *workspace;
    long workspace_floats;
};

__host__ __device__ inline int cnn_bwd_grid(int rows) { return rows < kCnnBwdMaxGrid ? rows : kCnnBwdMaxGrid; }

// the length of params / dparams
__host__ __device__ inline int cnn_param_count(int channels, int layers, const int *filters) {
    int n = 0, cin = channels;
    for (int l = 0; l < layers; ++l) n += filters[l] * cin * 16 + filters[l], cin = filters[l];
    return n;
}

// why the arguments cannot be served, or nullptr (cnn_capi.hip and the emulator share it); `check_buffers` off: the workspace query
inline const char *cnn_bwd_refusal(const CnnTrunkBwd &b, bool check_buffers) {
    CnnTrunk a = b.t;
    const int side = a.layers >= 1 && a.layers <= kCnnMaxLayers ? a.res >> a.layers : 0;
    if (!check_buffers) {                                     // the shape alone
        static const float dummy = 0.0f;
        a.x = a.params = a.mean = a.var = &dummy;
        a.ldx = kCnnMaxChannels * kCnnMaxRes * kCnnMaxRes;
    }
    a.out = const_cast<float *>(a.x), a.out_off = 0, a.ldo = kCnnMaxFilters * kCnnMaxRes * kCnnMaxRes;      // (no output operand here)
    if (const char *why = cnn_refusal(a)) return why;
    if (!check_buffers) return nullptr;
    if (!b.dout) return "dout is null";
    if (!b.dparams) return "dparams is null";
    if (!b.workspace) return "workspace is null";
    if (b.dout_off < 0) return "dout_off is negative";
    if (b.lddo < b.dout_off + a.filters[a.layers - 1] * side * side) return "lddo is smaller than dout_off plus the feature width";
    if (b.workspace_floats < (long)cnn_bwd_grid(a.rows) * cnn_param_count(a.channels, a.layers, a.filters))
        return "workspace_floats is smaller than emloco_cnn_trunk_backward_workspace asks for";
    return nullptr;
}

// cnn_conv over all eight waves: waves 4-7 take the rows from (n_rows + 1) / 2 on
__device__ __forceinline__ void cnn_conv8(const float *in, int cin, int in_plane, int in_wp, int in_slot, const float *__restrict__ w,
                                          const float *__restrict__ bias, int nf, int wave, int n_rows, int w_out, float *out, int o_plane,
                                          int o_row, int o_base) {
    const int h = (n_rows + 1) >> 1;
    const int ra = wave >= 4 ? h : 0, rb = wave >= 4 ? n_rows : h;
    cnn_conv(in, cin, in_plane, in_wp, in_slot + 2 * ra, w, bias, nf, wave & 3, rb - ra, w_out, out, o_plane, o_row, o_base + ra * o_row);
}

// this lane's place in a layer's weight-gradient split: lanes [first, first + lanes) of the workgroup share the layer
struct CnnOwn { int f, ci, share, shares; };
__device__ __forceinline__ CnnOwn cnn_own(int tid, int nf, int cin, int first, int lanes) {
    const bool in = tid >= first && tid < first + lanes;
    const int t = in ? tid - first : 0, pairs = nf * cin, pair = t % pairs;
    CnnOwn o;
    o.f = pair / cin, o.ci = pair - o.f * cin, o.shares = lanes / pairs, o.share = in ? t / pairs : o.shares;
    return o;
}

// acc[ky][kx] += d[f][oy][ox] * in[ci][2 oy - 1 + ky][2 ox - 1 + kx] over this lane's share of rows [0, n_rows) x columns [0, w_out).
// `d`: gradient image, value (f, oy, ox) at d[f * d_plane + oy * d_wp + ox + d_base]; `in`, `in_slot` as for cnn_conv.
__device__ __forceinline__ void cnn_wgrad(const CnnOwn o, const float *d, int d_plane, int d_wp, int d_base, const float *in, int in_plane,
                                          int in_wp, int in_slot, int n_rows, int w_out, float (&acc)[16], float &accb) {
    if (o.share >= o.shares) return;
    const float *dp = d + o.f * d_plane + d_base;
    const float *src = in + o.ci * in_plane + in_slot * in_wp;
    const int npix = n_rows * w_out;
#pragma unroll 1
    for (int p = o.share; p < npix; p += o.shares) {
        const int oy = p / w_out, ox = p - oy * w_out;
        const float g = dp[oy * d_wp + ox];
        const float *s = src + 2 * oy * in_wp + 2 * ox;
        accb += g;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const cnn_f2 lo = *reinterpret_cast<const cnn_f2 *>(s + ky * in_wp);
            const cnn_f2 hi = *reinterpret_cast<const cnn_f2 *>(s + ky * in_wp + 2);
            acc[ky * 4 + 0] = fmaf(g, lo.x, acc[ky * 4 + 0]);
            acc[ky * 4 + 1] = fmaf(g, lo.y, acc[ky * 4 + 1]);
            acc[ky * 4 + 2] = fmaf(g, hi.x, acc[ky * 4 + 2]);
            acc[ky * 4 + 3] = fmaf(g, hi.y, acc[ky * 4 + 3]);
        }
    }
}

// Gradient of rows [ya, yb) x columns [0, w) of the layer below, all `cin` channels, from the padded gradient image `d` (filters nf,
// plane d_plane, row d_wp, pixel (0, 0) at d_wp + 1) and the weights w[nf][cin][4][4]; masked by the layer's own value
// act[ci * a_plane + (y - ya) * a_wp + x + a_base] > 0; to out[ci * o_plane + (y - ya) * o_wp + x + o_base].
__device__ __forceinline__ void cnn_dgrad(const float *d, int nf, int d_plane, int d_wp, const float *__restrict__ w, int cin, int ya, int yb,
                                          int wd, const float *act, int a_plane, int a_wp, int a_base, float *out, int o_plane, int o_wp,
                                          int o_base) {
    const int per = (yb - ya) * wd, total = cin * per;
#pragma unroll 1
    for (int i = (int)threadIdx.x; i < total; i += kCnnBwdThreads) {
        const int ci = i / per, rem = i - ci * per, ry = rem / wd, x = rem - ry * wd, y = ya + ry;
        const int ky = (y + 1) & 1, kx = (x + 1) & 1;
        // padded coordinates of output pixel ((y + 1 - ky) / 2, (x + 1 - kx) / 2); taps ky + 2 / kx + 2 read the pixel before
        const float *dp = d + (((y + 1 - ky) >> 1) + 1) * d_wp + ((x + 1 - kx) >> 1) + 1;
        const float *wp = w + ci * 16 + ky * 4 + kx;
        float acc = 0.0f;
        for (int f = 0; f < nf; ++f) {
            const float *q = dp + f * d_plane, *k = wp + f * cin * 16;
            acc = fmaf(q[0], k[0], acc);
            acc = fmaf(q[-1], k[2], acc);
            acc = fmaf(q[-d_wp], k[8], acc);
            acc = fmaf(q[-d_wp - 1], k[10], acc);
        }
        out[ci * o_plane + ry * o_wp + x + o_base] = act[ci * a_plane + ry * a_wp + x + a_base] > 0.0f ? acc : 0.0f;
    }
}

// the shares of one layer summed in ascending order through `red` (LDS), into this workgroup's partial vector
__device__ __forceinline__ void cnn_bwd_fold(const CnnOwn o, int nf, int cin, const float (&acc)[16], float accb, float *red, float *part) {
    const int tid = (int)threadIdx.x, pairs = nf * cin;
    __syncthreads();                                          // (red is free: whoever read it last has passed)
    if (o.share < o.shares) {
#pragma unroll
        for (int t = 0; t < 16; ++t) red[(o.share * pairs + o.f * cin + o.ci) * 16 + t] = acc[t];
        if (o.ci == 0) red[kCnnBwdThreads * 16 + o.share * nf + o.f] = accb;
    }
    __syncthreads();
    for (int e = tid; e < pairs * 16; e += kCnnBwdThreads) {
        float s = 0.0f;
        for (int sh = 0; sh < o.shares; ++sh) s += red[sh * pairs * 16 + e];
        part[e] = s;
    }
    if (tid < nf) {
        float s = 0.0f;
        for (int sh = 0; sh < o.shares; ++sh) s += red[kCnnBwdThreads * 16 + sh * nf + tid];
        part[pairs * 16 + tid] = s;
    }
}

__global__ void __launch_bounds__(kCnnBwdThreads)
cnn_trunk_backward_kernel(const CnnTrunk a, const float *__restrict__ xin, const float *__restrict__ mean, const float *__restrict__ var,
                          const float *__restrict__ params, const float *__restrict__ doutp, int lddo, int dout_off,
                          float *__restrict__ workspace) {
    __shared__ __attribute__((aligned(16))) float s_mem[kBwdLdsFloats];
    float *s_in = s_mem + kBwdIn, *s_l1 = s_mem + kBwdL1, *s_l2 = s_mem + kBwdL2, *s_l3 = s_mem + kBwdL3, *s_l4 = s_mem + kBwdL4;
    float *s_d1 = s_mem + kBwdD1, *s_d2 = s_mem + kBwdD2, *s_d3 = s_mem + kBwdD3, *s_d4 = s_mem + kBwdD4;
    const int tid = (int)threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int H0 = a.res, H1 = H0 >> 1, H2 = H0 >> 2, H3 = H0 >> 3, H4 = H0 >> 4;
    const int C0 = a.channels, F1 = a.filters[0];
    // (layers the shape does not have: one filter, so that the ownership arithmetic stays defined; they are never accumulated into)
    const int F2 = a.layers >= 2 ? a.filters[1] : 1, F3 = a.layers >= 3 ? a.filters[2] : 1, F4 = a.layers >= 4 ? a.filters[3] : 1;
    const float *w1 = params, *b1 = w1 + F1 * C0 * 16;
    const float *w2 = b1 + F1, *b2 = w2 + F2 * F1 * 16;
    const float *w3 = b2 + F2, *b3 = w3 + F3 * F2 * 16;
    const float *w4 = b3 + F3, *b4 = w4 + F4 * F3 * 16;
    const int in_wp = H0 + 2, in_plane = kCnnInSlots * in_wp;
    const int l1_wp = H1 + 2, l1_plane = kCnnL1Slots * l1_wp;
    const int l2_wp = H2 + 2, l2_plane = (H2 + 2) * l2_wp;
    const int l3_wp = H3 + 2, l3_plane = (H3 + 2) * l3_wp;
    const int l4_wp = H4 + 2, l4_plane = (H4 + 2) * l4_wp;
    const int row_floats = H0 * C0;
    // layers 1 and 2 take all lanes; 3 and 4, a few pixels each, take one half of the workgroup each and share one set of accumulators
    const CnnOwn o1 = cnn_own(tid, F1, C0, 0, kCnnBwdThreads), o2 = cnn_own(tid, F2, F1, 0, kCnnBwdThreads);
    const CnnOwn o3 = cnn_own(tid, F3, F2, 0, kCnnBwdThreads / 2), o4 = cnn_own(tid, F4, F3, kCnnBwdThreads / 2, kCnnBwdThreads / 2);
    float g1[16], g2[16], g34[16], gb1 = 0.0f, gb2 = 0.0f, gb34 = 0.0f;
#pragma unroll
    for (int t = 0; t < 16; ++t) g1[t] = g2[t] = g34[t] = 0.0f;

    // the zero borders of every image are written here and never again
    for (int i = tid; i < kBwdLdsFloats; i += kCnnBwdThreads) s_mem[i] = 0.0f;
    __syncthreads();

    for (long row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const float *x = xin + row * a.ldx;
        const float *dout = doutp + row * lddo + dout_off;

        // input rows [2 la - 1, 2 lb + 1), normalised, into slots 0.. of s_in (cnn_trunk_kernel's stage_input)
        auto stage_input = [&](int la, int lb) {
            const int y0 = 2 * la - 1, total = (2 * (lb - la) + 2) * row_floats;
            for (int i = tid; i < total; i += kCnnBwdThreads) {
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
        // dout . [top > 0] into the padded gradient image of the top layer
        auto load_top = [&](float *d, const float *top, int nf, int h, int plane, int wp) {
            for (int i = tid; i < nf * h * h; i += kCnnBwdThreads) {
                const int f = i / (h * h), rem = i - f * h * h, y = rem / h, xx = rem - y * h;
                const int at = f * plane + (y + 1) * wp + xx + 1;
                d[at] = top[at] > 0.0f ? dout[i] : 0.0f;
            }
        };

        if (a.layers == 1) {
            for (int la = 0; la < H1; la += 2 * kCnnBand) {
                const int lb = la + 2 * kCnnBand < H1 ? la + 2 * kCnnBand : H1;
                stage_input(la, lb);
                __syncthreads();
                cnn_conv8(s_in, C0, in_plane, in_wp, 0, w1, b1, F1, wave, lb - la, H1, s_l1, l1_plane, l1_wp, 1);
                __syncthreads();
                for (int i = tid; i < F1 * (lb - la) * H1; i += kCnnBwdThreads) {
                    const int f = i / ((lb - la) * H1), rem = i - f * (lb - la) * H1, ry = rem / H1, xx = rem - ry * H1;
                    s_d1[f * kCnnD1Plane + ry * H1 + xx] = s_l1[f * l1_plane + ry * l1_wp + xx + 1] > 0.0f ? dout[f * H1 * H1 + (la + ry) * H1 + xx] : 0.0f;
                }
                __syncthreads();
                cnn_wgrad(o1, s_d1, kCnnD1Plane, H1, 0, s_in, in_plane, in_wp, 0, lb - la, H1, g1, gb1);
                __syncthreads();
            }
            continue;
        }

        // two sweeps over the bands: stage the input, the first-layer band; the second adds the backward work of the band
        for (int second = 0; second < 2; ++second) {
            for (int r0 = 0; r0 < H2; r0 += kCnnBand) {
                const int r1 = r0 + kCnnBand < H2 ? r0 + kCnnBand : H2;
                const int la = r0 == 0 ? 0 : 2 * r0 + 1;                      // (rows 2 r0 - 1 and 2 r0 were carried over)
                const int lb = 2 * r1 + 1 < H1 ? 2 * r1 + 1 : H1;
                stage_input(la, lb);
                if (r0 == 0)                                                  // row -1: padding
                    for (int i = tid; i < F1 * H1; i += kCnnBwdThreads) s_l1[(i / H1) * l1_plane + (i % H1) + 1] = 0.0f;
                if (2 * r1 == H1)                                             // row H1: padding
                    for (int i = tid; i < F1 * H1; i += kCnnBwdThreads)
                        s_l1[(i / H1) * l1_plane + (H1 - (2 * r0 - 1)) * l1_wp + (i % H1) + 1] = 0.0f;
                __syncthreads();
                const int slot = la - (2 * r0 - 1);                           // where first-layer row la sits
                cnn_conv8(s_in, C0, in_plane, in_wp, 0, w1, b1, F1, wave, lb - la, H1, s_l1, l1_plane, l1_wp, slot * l1_wp + 1);
                __syncthreads();
                if (!second) {
                    cnn_conv8(s_l1, F1, l1_plane, l1_wp, 0, w2, b2, F2, wave, r1 - r0, H2, s_l2, l2_plane, l2_wp, (r0 + 1) * l2_wp + 1);
                } else {
                    cnn_wgrad(o2, s_d2, l2_plane, l2_wp, (r0 + 1) * l2_wp + 1, s_l1, l1_plane, l1_wp, 0, r1 - r0, H2, g2, gb2);
                    cnn_dgrad(s_d2, F2, l2_plane, l2_wp, w2, F1, la, lb, H1, s_l1, l1_plane, l1_wp, slot * l1_wp + 1, s_d1, kCnnD1Plane, H1, 0);
                    __syncthreads();
                    cnn_wgrad(o1, s_d1, kCnnD1Plane, H1, 0, s_in, in_plane, in_wp, 0, lb - la, H1, g1, gb1);
                }
                __syncthreads();
                if (r1 < H2) {                                                // the next band's rows 2 r1 - 1 and 2 r1: slots 2 kCnnBand, + 1 -> 0, 1
                    for (int i = tid; i < F1 * 2 * H1; i += kCnnBwdThreads) {
                        const int f = i / (2 * H1), rem = i - f * 2 * H1, j = rem / H1, c = rem - j * H1;
                        s_l1[f * l1_plane + j * l1_wp + c + 1] = s_l1[f * l1_plane + (2 * kCnnBand + j) * l1_wp + c + 1];
                    }
                    __syncthreads();
                }
            }
            if (second) break;
            // between the sweeps: the upper layers forward, then back down to the second layer's gradient image
            if (a.layers >= 3) {
                cnn_conv8(s_l2, F2, l2_plane, l2_wp, 0, w3, b3, F3, wave, H3, H3, s_l3, l3_plane, l3_wp, l3_wp + 1);
                __syncthreads();
            }
            if (a.layers == 4) {
                cnn_conv8(s_l3, F3, l3_plane, l3_wp, 0, w4, b4, F4, wave, H4, H4, s_l4, l4_plane, l4_wp, l4_wp + 1);
                __syncthreads();
                load_top(s_d4, s_l4, F4, H4, l4_plane, l4_wp);
                __syncthreads();
                cnn_wgrad(o4, s_d4, l4_plane, l4_wp, l4_wp + 1, s_l3, l3_plane, l3_wp, 0, H4, H4, g34, gb34);
                cnn_dgrad(s_d4, F4, l4_plane, l4_wp, w4, F3, 0, H3, H3, s_l3, l3_plane, l3_wp, l3_wp + 1, s_d3, l3_plane, l3_wp, l3_wp + 1);
                __syncthreads();
            } else if (a.layers == 3) {
                load_top(s_d3, s_l3, F3, H3, l3_plane, l3_wp);
                __syncthreads();
            }
            if (a.layers >= 3) {
                cnn_wgrad(o3, s_d3, l3_plane, l3_wp, l3_wp + 1, s_l2, l2_plane, l2_wp, 0, H3, H3, g34, gb34);
                cnn_dgrad(s_d3, F3, l3_plane, l3_wp, w3, F2, 0, H2, H2, s_l2, l2_plane, l2_wp, l2_wp + 1, s_d2, l2_plane, l2_wp, l2_wp + 1);
                __syncthreads();
            } else {
                load_top(s_d2, s_l2, F2, H2, l2_plane, l2_wp);
                __syncthreads();
            }
        }
    }

    // the shares, then this workgroup's partial vector
    // (P spelt out: a loop over a.filters would index the kernel argument dynamically and put it in scratch)
    const int count = F1 * C0 * 16 + F1 + (a.layers >= 2 ? F2 * F1 * 16 + F2 : 0) + (a.layers >= 3 ? F3 * F2 * 16 + F3 : 0) +
                      (a.layers >= 4 ? F4 * F3 * 16 + F4 : 0);
    float *part = workspace + (long)blockIdx.x * count;
    cnn_bwd_fold(o1, F1, C0, g1, gb1, s_mem, part);
    part += F1 * C0 * 16 + F1;
    if (a.layers >= 2) cnn_bwd_fold(o2, F2, F1, g2, gb2, s_mem, part);
    part += F2 * F1 * 16 + F2;
    if (a.layers >= 3) cnn_bwd_fold(o3, F3, F2, g34, gb34, s_mem, part);
    part += F3 * F2 * 16 + F3;
    if (a.layers >= 4) cnn_bwd_fold(o4, F4, F3, g34, gb34, s_mem, part);
}

// dparams[e] = sum over blocks, ascending, of workspace[block][e]
__global__ void __launch_bounds__(256)
cnn_grad_reduce_kernel(const float *__restrict__ workspace, int blocks, int count, float *__restrict__ dparams) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= count) return;
    float s = 0.0f;
    for (int b = 0; b < blocks; ++b) s += workspace[(long)b * count + e];
    dparams[e] = s;
}

}  // namespace emloco
