// Fused Winograd F(2x2,3x3) convolution for gfx950 (CDNA4): stride-1
// 3x3, bf16 NCHW in and out, fp32 accumulation. The transform matrices
// are those of ops/winograd_ref.py (Lavin & Gray, arXiv:1509.09308).
//
//   U = G w G^T     wino_filter_kernel: fp32, rounded once to bf16, written
//                   as U[16][Kp][Cp] (channel-contiguous, zero padded)
//   V = B^T d B     main kernel, in registers, rounded once to bf16
//   M = U . V       16 GEMMs over C on mfma_f32_16x16x32_bf16
//   Y = A^T M A     main kernel, registers + one pass through LDS
//
// Neither V nor M touches global memory.
//
// Main kernel, per block (256 threads = 4 waves): KB output channels x a
// patch of 2x16 Winograd tiles (4 output rows x 32 output columns, read
// from a 6x34 input patch per channel) of one image.
//
// * Reduction over C in chunks of 32 (the MFMA k). Thread (tile t, channel
//   quad q) loads its 4x4 input window of 4 channels with clamped,
//   always-in-bounds addresses and zeroes pads and tails with bit masks in
//   the transform: there is no padded copy of x and the loads of a chunk
//   stay in flight together. It forms V in fp32 and writes 16 x 8 bytes
//   into the LDS image [16 positions][32 tiles][32 channels]; the four
//   16-byte channel groups of a tile row are XOR-swizzled with (tile>>2)&3
//   so a B fragment is one conflict-free ds_read_b128 per lane. The image
//   is double buffered: chunk n+1 is loaded and transformed around the
//   MFMAs of chunk n, one barrier per chunk.
// * Wave i owns positions (i, 0..3) of the 4x4 transform domain over the
//   whole KB x 32-tile block tile, so a U fragment is used by one wave
//   only: it goes from global memory (L2) straight into registers as
//   16-byte loads, one chunk ahead. Per chunk a wave issues 4*(KB/16)*2
//   MFMAs and holds 4*(KB/16)*2*4 accumulators.
// * Epilogue: each wave applies the right-hand output transform to its
//   row in registers (P_i[0] = M_i0+M_i1+M_i2, P_i[1] = M_i1-M_i2-M_i3)
//   and writes P_i as fp32 into the LDS the V buffers no longer need
//   (row stride padded to 68 floats: the wave's 8-byte writes then cover
//   every bank exactly twice). After one barrier the block combines
//   Y[0] = P_0+P_1+P_2, Y[1] = P_1-P_2-P_3, adds the bias, rounds to bf16
//   (nearest even) and stores 16-byte row segments where OW % 8 == 0 and
//   the segment is whole, guarded scalars otherwise.
// * No atomics, fixed summation order: results are bit-identical from run
//   to run. No synchronisation, no allocation outside torch's allocator.
//
// The data-gradient is the same kernel on the output gradient with the
// filter of output channel c and input channel k read as
// w[k][c][2-r][2-s]; wino_filter_kernel does that with `transposed`.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cstdint>
#include <string>

namespace conv_wino {

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr int CK = 32;        // channels per chunk (MFMA k)
constexpr int TILES = 32;     // 2 x 16 Winograd tiles per block
constexpr int KPAD = 64;      // U's K padding (the largest KB)
constexpr int PROW = 68;      // floats per (wave, k) row of the P image
constexpr int VBUF = 16 * TILES * CK;  // shorts per V buffer

struct WinoGeom {
  int N, C, H, W;   // input (C is the reduction dim of this launch)
  int K;            // output channels of this launch
  int OH, OW, ph, pw;
  int Kp, Cp;       // padded extents of U
  int row_blocks, col_blocks;
};

// Scalar fp32 only in this file: the packed fp32 forms are kept out of it.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

__device__ __forceinline__ float bf2f(unsigned short v) {
  return __uint_as_float((unsigned)v << 16);
}

// two floats -> two bf16 (round to nearest even) in one dword, lo first
__device__ __forceinline__ int pack_bf16(float lo, float hi) {
  f32x2 v = {lo, hi};
  bf16x2 r = __builtin_convertvector(v, bf16x2);
  return __builtin_bit_cast(int, r);
}

// ---------------------------------------------------------------------------
// Filter transform: U[p][ko][cr] = (G g G^T)[p], g the 3x3 filter of output
// channel ko and reduction channel cr; zero where ko or cr is padding.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void wino_filter_kernel(
    const unsigned short* __restrict__ w, unsigned short* __restrict__ U,
    int Kw, int Cw, int Kout, int Cred, int Kp, int Cp, int transposed) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)Kp * Cp) return;
  const int cr = (int)(idx % Cp);
  const int ko = (int)(idx / Cp);
  float u[4][4];
  if (ko < Kout && cr < Cred) {
    float g[3][3];
    // w is [Kw][Cw][3][3]; transposed: filter (ko=c, cr=k), rotated 180
    const unsigned short* src =
        transposed ? w + ((int64_t)cr * Cw + ko) * 9
                   : w + ((int64_t)ko * Cw + cr) * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s)
        g[r][s] = bf2f(transposed ? src[(2 - r) * 3 + (2 - s)] : src[r * 3 + s]);
    float t[4][3];  // G g
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const float e = g[0][s] + g[2][s];
      t[0][s] = g[0][s];
      t[1][s] = 0.5f * (e + g[1][s]);
      t[2][s] = 0.5f * (e - g[1][s]);
      t[3][s] = g[2][s];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // (G g) G^T
      const float e = t[i][0] + t[i][2];
      u[i][0] = t[i][0];
      u[i][1] = 0.5f * (e + t[i][1]);
      u[i][2] = 0.5f * (e - t[i][1]);
      u[i][3] = t[i][2];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) u[i][j] = 0.f;
  }
  const int64_t plane = (int64_t)Kp * Cp;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      U[(i * 4 + j) * plane + idx] =
          (unsigned short)(pack_bf16(u[i][j], 0.f) & 0xffff);
}

// ---------------------------------------------------------------------------
// Main kernel
// ---------------------------------------------------------------------------

template <int KB>
__global__ __launch_bounds__(256) void wino_fwd_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ U,
    const float* __restrict__ bias, unsigned short* __restrict__ out,
    WinoGeom g) {
  constexpr int KF = KB / 16;  // 16-row MFMA fragments per block tile
  static_assert(4 * KB * PROW * 4 <= (2 * VBUF + 2048) * 2,
                "P image must fit the LDS declared below");

  // block -> (k tile, column block, row block, image), XCD-aware bijective
  // swizzle as in conv_fwd_kernel
  const int k_tiles = (g.K + KB - 1) / KB;
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int xcd = blockIdx.x & 7, sub = blockIdx.x >> 3;
  int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + sub;
  if (bid >= nwg) bid = blockIdx.x;  // never taken: the mapping is bijective
  const int kt = bid % k_tiles;
  bid /= k_tiles;
  const int cb = bid % g.col_blocks;
  bid /= g.col_blocks;
  const int rb = bid % g.row_blocks;
  const int n = bid / g.row_blocks;

  const int k0 = kt * KB;
  const int oh0 = rb * 4, ow0 = cb * 32;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  // V double buffer (2 x 32 KiB); the epilogue's P image (4*KB*PROW floats,
  // 68 KiB at KB = 64) overlays it
  __shared__ __attribute__((aligned(16))) short lds[2 * VBUF + 2048];

  // ---- input window of this thread: tile t, channels 4q..4q+3 -------------
  const int t = tid & 31, q = tid >> 5;
  const int ty = t >> 4, tx = t & 15;
  int off[16];      // offset in the channel plane, clamped to 0 where invalid
  unsigned okm[16];  // all ones where the element exists, 0 in the padding
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ih = oh0 + 2 * ty - g.ph + r;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int iw = ow0 + 2 * tx - g.pw + s;
      const bool ok = ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
      okm[r * 4 + s] = ok ? ~0u : 0u;
      off[r * 4 + s] = ok ? ih * g.W + iw : 0;
    }
  }
  const int64_t HW = (int64_t)g.H * g.W;
  const unsigned short* xn = x + (int64_t)n * g.C * HW;
  // LDS dword index of this thread's 8 bytes within a position's image
  const int vw = t * 16 + (((q >> 1) ^ ((t >> 2) & 3)) << 2) + ((q & 1) << 1);

  // One dword per element and no use of the values here: the 64 loads of a
  // chunk stay in flight together (selecting or packing at the load made
  // the compiler wait for each one in turn).
  unsigned raw[4][16];
  auto load_raw = [&](int c0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + q * 4 + e;
      const unsigned short* src = xn + (int64_t)(c < g.C ? c : g.C - 1) * HW;
#pragma unroll
      for (int i = 0; i < 16; ++i) raw[e][i] = src[off[i]];  // always inside x
    }
  };
  // V = B^T d B of the four channels of chunk c0, rounded once to bf16, into
  // `buf`; pads and the channel tail become zeros here
  auto transform = [&](int buf, int c0) {
    float v[4][16];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned cvm = c0 + q * 4 + e < g.C ? ~0u : 0u;
      float d[4][4], b[4][4];
#pragma unroll
      for (int i = 0; i < 16; ++i)  // masks, not selects: no branches
        d[i >> 2][i & 3] = __uint_as_float((raw[e][i] & okm[i] & cvm) << 16);
#pragma unroll
      for (int s = 0; s < 4; ++s) {  // B^T d
        b[0][s] = d[0][s] - d[2][s];
        b[1][s] = d[1][s] + d[2][s];
        b[2][s] = d[2][s] - d[1][s];
        b[3][s] = d[1][s] - d[3][s];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // (B^T d) B
        v[e][r * 4 + 0] = b[r][0] - b[r][2];
        v[e][r * 4 + 1] = b[r][1] + b[r][2];
        v[e][r * 4 + 2] = b[r][2] - b[r][1];
        v[e][r * 4 + 3] = b[r][1] - b[r][3];
      }
    }
    int* dst = (int*)(lds + buf * VBUF) + vw;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      i32x2 pk = {pack_bf16(v[0][p], v[1][p]), pack_bf16(v[2][p], v[3][p])};
      *(i32x2*)(dst + p * (TILES * CK / 2)) = pk;
    }
  };

  // ---- U fragments of this wave: positions wid*4 + j ----------------------
  // lane: row k0 + kf*16 + (lane & 15), channels c0 + (lane >> 4)*8 .. +8
  const int64_t uplane = (int64_t)g.Kp * g.Cp;
  const unsigned short* ub =
      U + (int64_t)(wid * 4) * uplane +
      (int64_t)(k0 + (lane & 15)) * g.Cp + ((lane >> 4) << 3);
  auto load_u = [&](s16x8 (&a)[4][KF], int c0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int kf = 0; kf < KF; ++kf)
        a[j][kf] = *(const s16x8*)(ub + j * uplane +
                                   (int64_t)(kf * 16) * g.Cp + c0);
  };
  // B fragment: tile nf*16 + (lane & 15), channel group lane >> 4
  int boff[2];
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    const int bt = nf * 16 + (lane & 15);
    boff[nf] = bt * CK + (((lane >> 4) ^ ((bt >> 2) & 3)) << 3);
  }

  f32x4 acc[4][KF][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int kf = 0; kf < KF; ++kf)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) acc[j][kf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  s16x8 a_cur[4][KF], a_nxt[4][KF];
  load_raw(0);
  load_u(a_cur, 0);
  transform(0, 0);
  __syncthreads();

  const int chunks = g.Cp / CK;
  for (int ch = 0; ch < chunks; ++ch) {
    const int buf = ch & 1;
    const bool more = ch + 1 < chunks;
    if (more) {
      load_raw((ch + 1) * CK);
      load_u(a_nxt, (ch + 1) * CK);
    }
    const short* vb = lds + buf * VBUF + (wid * 4) * (TILES * CK);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s16x8 bfrag[2];
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
        bfrag[nf] = *(const s16x8*)(vb + j * (TILES * CK) + boff[nf]);
#pragma unroll
      for (int kf = 0; kf < KF; ++kf)
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
          acc[j][kf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_cur[j][kf], bfrag[nf], acc[j][kf][nf], 0, 0, 0);
    }
    if (more) {
      transform(buf ^ 1, (ch + 1) * CK);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int kf = 0; kf < KF; ++kf) a_cur[j][kf] = a_nxt[j][kf];
    }
    __syncthreads();
  }

  // ---- epilogue -------------------------------------------------------------
  // P image: [wave][k][tile][2] fp32, k rows PROW floats apart. D layout of
  // the MFMA: row (lane >> 4)*4 + reg, column lane & 15.
  float* P = (float*)lds;
#pragma unroll
  for (int kf = 0; kf < KF; ++kf)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float m0 = acc[0][kf][nf][reg], m1 = acc[1][kf][nf][reg];
        const float m2 = acc[2][kf][nf][reg], m3 = acc[3][kf][nf][reg];
        f32x2 p = {m0 + m1 + m2, m1 - m2 - m3};
        const int k = kf * 16 + ((lane >> 4) << 2) + reg;
        const int tile = nf * 16 + (lane & 15);
        *(f32x2*)(P + (wid * KB + k) * PROW + tile * 2) = p;
      }
  __syncthreads();

  // item = (k, tile row ty, 4-tile segment): two output rows x 8 columns
  const bool vec_rows = (g.OW & 7) == 0;
  const int64_t OHW = (int64_t)g.OH * g.OW;
#pragma unroll
  for (int it = 0; it < KB * 8 / 256; ++it) {
    const int idx = it * 256 + tid;
    const int seg = idx & 3, ity = (idx >> 2) & 1, k = idx >> 3;
    const int kout = k0 + k;
    const int ow = ow0 + seg * 8;
    if (kout >= g.K || ow >= g.OW) continue;
    float y0[8], y1[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* src = P + k * PROW + (ity * 16 + seg * 4) * 2 + h * 4;
      const f32x4 p0 = *(const f32x4*)(src);
      const f32x4 p1 = *(const f32x4*)(src + 1 * KB * PROW);
      const f32x4 p2 = *(const f32x4*)(src + 2 * KB * PROW);
      const f32x4 p3 = *(const f32x4*)(src + 3 * KB * PROW);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        y0[h * 4 + e] = p0[e] + p1[e] + p2[e];
        y1[h * 4 + e] = p1[e] - p2[e] - p3[e];
      }
    }
    const float b = bias ? bias[kout] : 0.f;
    unsigned short* obase = out + ((int64_t)n * g.K + kout) * OHW;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int oh = oh0 + ity * 2 + p;
      if (oh >= g.OH) continue;
      const float* y = p ? y1 : y0;
      unsigned short* dst = obase + (int64_t)oh * g.OW + ow;
      if (vec_rows && ow + 8 <= g.OW) {
        i32x4 pk = {pack_bf16(y[0] + b, y[1] + b), pack_bf16(y[2] + b, y[3] + b),
                    pack_bf16(y[4] + b, y[5] + b), pack_bf16(y[6] + b, y[7] + b)};
        *(i32x4*)dst = pk;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (ow + e < g.OW)
            dst[e] = (unsigned short)(pack_bf16(y[e] + b, 0.f) & 0xffff);
      }
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------

static WinoGeom make_geom(int64_t N, int64_t C, int64_t K, int64_t H,
                          int64_t W, int64_t ph, int64_t pw) {
  TORCH_CHECK(N >= 1 && C >= 1 && K >= 1 && H >= 1 && W >= 1,
              "wino_fwd: N, C, K, H, W must be positive");
  TORCH_CHECK(ph >= 0 && ph <= 2 && pw >= 0 && pw <= 2,
              "wino_fwd: padding must be 0, 1 or 2 per dimension, got (", ph,
              ", ", pw, ")");
  TORCH_CHECK(H + 2 * ph >= 3 && W + 2 * pw >= 3,
              "wino_fwd: the padded input is smaller than the 3x3 filter");
  TORCH_CHECK(H * W < (1LL << 31) && C < (1LL << 24) && K < (1LL << 24),
              "wino_fwd: problem too large");
  WinoGeom g;
  g.N = (int)N; g.C = (int)C; g.K = (int)K; g.H = (int)H; g.W = (int)W;
  g.ph = (int)ph; g.pw = (int)pw;
  g.OH = g.H + 2 * g.ph - 2;
  g.OW = g.W + 2 * g.pw - 2;
  g.Kp = (g.K + KPAD - 1) / KPAD * KPAD;
  g.Cp = (g.C + CK - 1) / CK * CK;
  g.row_blocks = (g.OH + 3) / 4;
  g.col_blocks = (g.OW + 31) / 32;
  return g;
}

// The instantiation of a problem: the only place that decides it.
struct WinoChoice {
  using Kern = void (*)(const unsigned short*, const unsigned short*,
                        const float*, unsigned short*, WinoGeom);
  Kern kern;
  int kb;
  std::string label;
};

static WinoChoice choose(const WinoGeom& g) {
  // K <= 32 would leave half of the 64-row tile masked
  if (g.K <= 32) return {wino_fwd_kernel<32>, 32, "wino<32>"};
  return {wino_fwd_kernel<64>, 64, "wino<64>"};
}

std::string wino_kernel_name(int64_t C, int64_t K, int64_t H, int64_t W,
                             int64_t ph, int64_t pw) {
  return choose(make_geom(1, C, K, H, W, ph, pw)).label;
}

torch::Tensor wino_fwd(torch::Tensor x, torch::Tensor w,
                       c10::optional<torch::Tensor> bias, int64_t ph,
                       int64_t pw, bool transposed) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.get_device() == w.get_device(),
              "wino_fwd: x and w must be on one GPU");
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && x.is_contiguous() &&
                  w.is_contiguous(),
              "wino_fwd: x and w must be contiguous 4-d tensors");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
                  w.scalar_type() == torch::kBFloat16,
              "wino_fwd: bf16 only");
  TORCH_CHECK(w.size(2) == 3 && w.size(3) == 3,
              "wino_fwd: 3x3 filters only (stride 1, dilation 1, groups 1), "
              "got ", w.size(2), "x", w.size(3));
  const int64_t Kw = w.size(0), Cw = w.size(1);
  const int64_t Cred = transposed ? Kw : Cw, Kout = transposed ? Cw : Kw;
  TORCH_CHECK(x.size(1) == Cred, "wino_fwd: channel mismatch: x has ",
              x.size(1), ", the filter reduces over ", Cred);
  const WinoGeom g =
      make_geom(x.size(0), Cred, Kout, x.size(2), x.size(3), ph, pw);
  const float* bptr = nullptr;
  torch::Tensor b32;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->numel() == Kout,
                "wino_fwd: bias must hold one value per output channel");
    b32 = bias->to(torch::kFloat).contiguous();
    bptr = b32.data_ptr<float>();
  }
  auto out = torch::empty({g.N, g.K, g.OH, g.OW}, x.options());
  auto U = torch::empty({16, g.Kp, g.Cp}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const int64_t fblocks = ((int64_t)g.Kp * g.Cp + 255) / 256;
  const WinoChoice ch = choose(g);
  const int64_t blocks = (int64_t)((g.K + ch.kb - 1) / ch.kb) * g.row_blocks *
                         g.col_blocks * g.N;
  TORCH_CHECK(fblocks < (1LL << 31) && blocks < (1LL << 31),
              "wino_fwd: grid too large");
  hipLaunchKernelGGL(wino_filter_kernel, dim3((uint32_t)fblocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)w.data_ptr(),
                     (unsigned short*)U.data_ptr(), (int)Kw, (int)Cw, g.K, g.C,
                     g.Kp, g.Cp, transposed ? 1 : 0);
  hipLaunchKernelGGL(ch.kern, dim3((uint32_t)blocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)x.data_ptr(),
                     (const unsigned short*)U.data_ptr(), bptr,
                     (unsigned short*)out.data_ptr(), g);
  return out;
}

}  // namespace conv_wino

void register_conv_wino(pybind11::module_& m) {
  m.def("wino_fwd", &conv_wino::wino_fwd, pybind11::arg("x"),
        pybind11::arg("w"), pybind11::arg("bias"), pybind11::arg("ph"),
        pybind11::arg("pw"), pybind11::arg("transposed") = false,
        "fused Winograd F(2x2,3x3) stride-1 conv (bf16 NCHW); transposed: x is "
        "the output gradient, w the forward weight, the result the data "
        "gradient");
  m.def("wino_kernel_name", &conv_wino::wino_kernel_name,
        "label of the kernel wino_fwd launches for (C, K, H, W, ph, pw); no "
        "tensor, no HIP call");
}
