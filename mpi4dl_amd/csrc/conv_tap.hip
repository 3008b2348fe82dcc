// Tap-shift direct convolution for gfx950 (CDNA4): stride-1 1x7, 7x1 and
// 3x3, bf16 NCHW in and out, fp32 accumulation, dilation 1, groups 1.
//
// Every input element is staged into LDS once, channel-innermost, and every
// filter tap is an address offset into that one image: no shifted copies, no
// transposing reads, no reload per tap.
//
//   tap_filter_kernel   w[K][C][R][S] -> Wt[R*S][Kp][Cp] bf16, zero padded
//                       (Kp = K up to 16, Cp = C up to 32), so the MFMA A
//                       fragment of one tap (16 output channels x 8 input
//                       channels) is one 16-byte read per lane. `transposed`
//                       reads w[c][k][R-1-r][S-1-s]: the data-grad's filter.
//   tap_fwd_kernel<R, S, MF, ALIGNED>
//
// Main kernel, per block (256 threads = 4 waves): MF*16 output channels x a
// TH x TW pixel tile of one image (4 x 64 for 1x7, 8 x 32 for 7x1 and 3x3).
//
// * The MFMA is mfma_f32_16x16x32_bf16 with its k over 32 input channels of
//   ONE tap. A B fragment is 16 consecutive columns of one tile row; the 16
//   fragments of the tile are split four per wave, and every wave holds all
//   MF row fragments: a weight fragment feeds 4 MFMAs and a pixel fragment MF
//   from registers.
// * Patch: per chunk of 32 channels the (TH+R-1) x PWL input patch sits in LDS
//   as [row][col][32 ch] with a pixel stride of 80 bytes (32 channels + 16
//   bytes of padding: the 16 lanes of a ds_read_b128 group then start on 16
//   disjoint 4-bank spans at every constant offset, so every tap shift reads
//   without conflicts). Patch column lc is input column ow0 - PADL + lc with
//   PADL = 8 where S > 1, and PWL is the needed width rounded up to whole
//   8-pixel groups (80 / 32 / 48 columns), so that on the ALIGNED path a
//   16-byte global load never straddles the patch edge.
//   Tap (r, s) of fragment (row, col0) is the ds_read_b128 at
//   ((row + r) * PWL + col0 + (lane & 15) + PADL - pw + s) * 80 B
//   + (lane >> 4) * 16 B.
// * Staging. ALIGNED (W % 8 == 0, 16-byte aligned x): a thread loads 16 bytes
//   (8 pixels) from each of 8 channels, transposes the 8x8 block of 16-bit
//   values with v_perm_b32 and writes eight ds_write_b128. Otherwise a thread
//   loads the 8 channels of one pixel as 2-byte elements and writes one
//   ds_write_b128 per pixel. Addresses are clamped into x; borders, pads and
//   the channel tail become zeros by masks applied after the loads, when the
//   values are packed for LDS. The patch is double buffered: the loads of
//   chunk i+1 are issued before the MFMAs of chunk i and written to the other
//   buffer after them; one barrier per chunk.
// * Weight fragments go from global memory (L2) straight into registers as
//   16-byte loads, one tap ahead of the MFMAs that use them.
// * Epilogue: bias, round to bf16 (nearest even), through an LDS image
//   [k][pixel] that overlays the patch buffers, then 16-byte row stores where
//   OW % 8 == 0, guarded element stores otherwise.
// * No atomics, fixed summation order: bit-identical from run to run. No
//   synchronisation, no host read, no allocation outside torch's allocator.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cstdint>
#include <string>

namespace conv_tap {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr int CK = 32;    // channels per chunk (MFMA k)
constexpr int PSTR = 40;  // shorts per patch pixel: 32 channels + 8 of padding

struct TapGeom {
  int N, C, H, W;  // input (C is the reduction dim of this launch)
  int K;           // output channels of this launch
  int OH, OW, ph, pw;
  int Kp, Cp;      // padded extents of Wt
  int row_blocks, col_blocks, k_tiles;
  int vec_out;     // 16-byte row stores are possible
};

// Tile geometry of a filter shape, shared by the kernel and the host.
template <int R, int S>
struct Tile {
  static constexpr int TH = S == 7 ? 4 : 8;
  static constexpr int TW = S == 7 ? 64 : 32;
  static constexpr int PH = TH + R - 1;
  static constexpr int PADL = S > 1 ? 8 : 0;              // columns left of ow0
  static constexpr int PWN = TW + S - 1;                  // columns needed
  static constexpr int PWL = (PADL + PWN + 7) / 8 * 8;    // columns in LDS
  static constexpr int PBUF = PH * PWL * PSTR;            // shorts per buffer
  static constexpr int ES = TH * TW + 8;                  // epilogue row stride
};

// Scalar fp32 only in this file: the packed fp32 forms are kept out of it.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// two floats -> two bf16 (round to nearest even) in one dword, lo first
__device__ __forceinline__ int pack_bf16(float lo, float hi) {
  f32x2 v = {lo, hi};
  bf16x2 r = __builtin_convertvector(v, bf16x2);
  return __builtin_bit_cast(int, r);
}

// ---------------------------------------------------------------------------
// Filter pre-pass: Wt[t][ko][cr] = the tap t = r*S + s of the filter of output
// channel ko and reduction channel cr; zero where ko or cr is padding.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void tap_filter_kernel(
    const unsigned short* __restrict__ w, unsigned short* __restrict__ Wt,
    int Cw, int Kout, int Cred, int Kp, int Cp, int RS, int transposed) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t plane = (int64_t)Kp * Cp;
  if (idx >= plane) return;
  const int cr = (int)(idx % Cp);
  const int ko = (int)(idx / Cp);
  const bool real = ko < Kout && cr < Cred;
  // w is [Kw][Cw][R][S]; transposed: filter (ko = c, cr = k), rotated 180
  const unsigned short* src =
      !real ? w
            : transposed ? w + ((int64_t)cr * Cw + ko) * RS
                         : w + ((int64_t)ko * Cw + cr) * RS;
  for (int t = 0; t < RS; ++t) {
    const unsigned short v = real ? src[transposed ? RS - 1 - t : t] : 0;
    Wt[t * plane + idx] = v;
  }
}

// ---------------------------------------------------------------------------
// Main kernel
// ---------------------------------------------------------------------------

template <int R, int S, int MF, bool ALIGNED>
__global__ __launch_bounds__(256) void tap_fwd_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ Wt,
    const float* __restrict__ bias, unsigned short* __restrict__ out,
    TapGeom g) {
  using T = Tile<R, S>;
  constexpr int TH = T::TH, TW = T::TW, PH = T::PH, PADL = T::PADL;
  constexpr int PWN = T::PWN, PWL = T::PWL, PBUF = T::PBUF, ES = T::ES;
  constexpr int RS = R * S;
  constexpr int KB = MF * 16;         // output channels per block
  constexpr int FPR = TW / 16;        // fragments per tile row
  constexpr int NF = TH * FPR / 4;    // fragments per wave
  static_assert(NF == 4, "16 fragments per tile, four per wave");
  constexpr int LDS_SHORTS = 2 * PBUF > KB * ES ? 2 * PBUF : KB * ES;

  // block -> (k tile, column block, row block, image), XCD-aware bijective
  // swizzle as in conv_fwd_kernel
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int xcd = blockIdx.x & 7, sub = blockIdx.x >> 3;
  int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + sub;
  if (bid >= nwg) bid = blockIdx.x;  // never taken: the mapping is bijective
  const int kt = bid % g.k_tiles;
  bid /= g.k_tiles;
  const int cb = bid % g.col_blocks;
  bid /= g.col_blocks;
  const int rb = bid % g.row_blocks;
  const int n = bid / g.row_blocks;

  const int k0 = kt * KB;
  const int oh0 = rb * TH, ow0 = cb * TW;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  // patch double buffer; the epilogue's [k][pixel] image overlays it
  __shared__ __attribute__((aligned(16))) short lds[LDS_SHORTS];

  const int64_t HW = (int64_t)g.H * g.W;
  const unsigned short* xn = x + (int64_t)n * g.C * HW;

  // ---- staging: what this thread loads of every chunk ----------------------
  // ALIGNED: one task = (patch row, 8-pixel group, 8-channel group).
  // Otherwise: UPT units = (patch row, needed column, 8-channel group).
  constexpr int G = PWL / 8;
  constexpr int TASKS = PH * G * 4;
  constexpr int UNITS = PH * PWN * 4;
  constexpr int UPT = (UNITS + 255) / 256;
  static_assert(TASKS <= 256, "one aligned task per thread");
  constexpr int NU = ALIGNED ? 1 : UPT;
  int soff[NU];       // offset in the channel plane, 0 where outside the image
  unsigned smask[NU];  // all ones inside the image, 0 in the padding
  int sdst[NU];       // LDS short index of the first write, -1: nothing to do
  int scg[NU];        // 8-channel group
  if constexpr (ALIGNED) {
    const int cg = tid & 3, gg = (tid >> 2) % G, pr = (tid >> 2) / G;
    const int ih = oh0 - g.ph + pr, iw = ow0 - PADL + gg * 8;
    // W % 8 == 0 and iw % 8 == 0: a group is wholly inside or outside
    const bool ok = tid < TASKS && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
    soff[0] = ok ? ih * g.W + iw : 0;
    smask[0] = ok ? ~0u : 0u;
    sdst[0] = tid < TASKS ? (pr * PWL + gg * 8) * PSTR + cg * 8 : -1;
    scg[0] = cg;
  } else {
#pragma unroll
    for (int it = 0; it < UPT; ++it) {
      const int u = it * 256 + tid;
      const int lcn = u % PWN, v = u / PWN;
      const int cg = v & 3, pr = v >> 2;
      const int ih = oh0 - g.ph + pr, iw = ow0 - g.pw + lcn;
      const bool ok = u < UNITS && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
      soff[it] = ok ? ih * g.W + iw : 0;
      smask[it] = ok ? ~0u : 0u;
      sdst[it] = u < UNITS ? (pr * PWL + PADL - g.pw + lcn) * PSTR + cg * 8 : -1;
      scg[it] = cg;
    }
  }

  // The loads of a chunk are issued together and not touched until `commit`:
  // masks there, no select at the load.
  i32x4 rawv[ALIGNED ? 8 : 1];
  unsigned raws[ALIGNED ? 1 : UPT][8];
  auto stage_load = [&](int c0) {
    if constexpr (ALIGNED) {
      if (sdst[0] >= 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int c = c0 + scg[0] * 8 + e;
          rawv[e] = *(const i32x4*)(xn + (int64_t)(c < g.C ? c : g.C - 1) * HW +
                                    soff[0]);  // always inside x
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < UPT; ++it) {
        if (sdst[it] < 0) continue;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int c = c0 + scg[it] * 8 + e;
          raws[it][e] = xn[(int64_t)(c < g.C ? c : g.C - 1) * HW + soff[it]];
        }
      }
    }
  };
  // channel-pair masks of a unit: dword j holds channels 2j (low), 2j+1
  auto pair_masks = [&](unsigned (&cm)[4], int c0, int cg, unsigned sm) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + cg * 8 + 2 * j;
      cm[j] = sm & ((c < g.C ? 0xffffu : 0u) | (c + 1 < g.C ? 0xffff0000u : 0u));
    }
  };
  auto stage_commit = [&](int buf, int c0) {
    short* pb = lds + buf * PBUF;
    if constexpr (ALIGNED) {
      if (sdst[0] < 0) return;
      unsigned cm[4];
      pair_masks(cm, c0, scg[0], smask[0]);
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        // 8x8 transpose of 16-bit values: pixel p of channels 2j and 2j+1
        const unsigned sel = (p & 1) ? 0x07060302u : 0x05040100u;
        i32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = (int)(__builtin_amdgcn_perm((unsigned)rawv[2 * j + 1][p >> 1],
                                             (unsigned)rawv[2 * j][p >> 1],
                                             sel) & cm[j]);
        *(i32x4*)(pb + sdst[0] + p * PSTR) = o;
      }
    } else {
#pragma unroll
      for (int it = 0; it < UPT; ++it) {
        if (sdst[it] < 0) continue;
        unsigned cm[4];
        pair_masks(cm, c0, scg[it], smask[it]);
        i32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = (int)((raws[it][2 * j] | (raws[it][2 * j + 1] << 16)) & cm[j]);
        *(i32x4*)(pb + sdst[it]) = o;
      }
    }
  };

  // ---- weight fragments: row k0 + mf*16 + (lane & 15), channels
  // c0 + (lane >> 4)*8 .. +8 of tap t. Rows past Kp (the tile's own padding)
  // are clamped: their results are never stored. ------------------------------
  const int64_t wplane = (int64_t)g.Kp * g.Cp;
  int64_t wrow[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int row = k0 + mf * 16 + (lane & 15);
    wrow[mf] = (int64_t)(row < g.Kp ? row : g.Kp - 1) * g.Cp + ((lane >> 4) << 3);
  }
  auto load_a = [&](s16x8 (&a)[MF], int t, int c0) {
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
      a[mf] = *(const s16x8*)(Wt + t * wplane + wrow[mf] + c0);
  };

  // B fragment nf of this wave: tile row frow, columns col0 .. col0 + 15
  int boff[NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const int f = wid * NF + nf;
    const int frow = f / FPR, col0 = (f % FPR) * 16;
    boff[nf] = (frow * PWL + col0 + (lane & 15) + PADL - g.pw) * PSTR +
               ((lane >> 4) << 3);
  }

  f32x4 acc[MF][NF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  s16x8 a_cur[MF], a_nxt[MF];
  stage_load(0);
  load_a(a_cur, 0, 0);
  stage_commit(0, 0);
  __syncthreads();

  const int chunks = g.Cp / CK;
  for (int ch = 0; ch < chunks; ++ch) {
    const int buf = ch & 1;
    const bool more = ch + 1 < chunks;
    if (more) stage_load((ch + 1) * CK);
    const short* pb = lds + buf * PBUF;
#pragma unroll
    for (int t = 0; t < RS; ++t) {
      if (t + 1 < RS)
        load_a(a_nxt, t + 1, ch * CK);
      else if (more)
        load_a(a_nxt, 0, (ch + 1) * CK);
      s16x8 bfrag[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        bfrag[nf] = *(const s16x8*)(pb + boff[nf] +
                                    ((t / S) * PWL + (t % S)) * PSTR);
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_cur[mf], bfrag[nf], acc[mf][nf], 0, 0, 0);
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) a_cur[mf] = a_nxt[mf];
    }
    if (more) stage_commit(buf ^ 1, (ch + 1) * CK);
    __syncthreads();
  }

  // ---- epilogue --------------------------------------------------------------
  // E image: [k][pixel] bf16, rows ES shorts apart. D layout of the MFMA: row
  // (lane >> 4)*4 + reg, column lane & 15.
  unsigned short* E = (unsigned short*)lds;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = mf * 16 + ((lane >> 4) << 2) + reg;
      const int kout = k0 + k;
      const float b = bias ? bias[kout < g.K ? kout : g.K - 1] : 0.f;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const int f = wid * NF + nf;
        const int pix = (f / FPR) * TW + (f % FPR) * 16 + (lane & 15);
        E[k * ES + pix] =
            (unsigned short)(pack_bf16(acc[mf][nf][reg] + b, 0.f) & 0xffff);
      }
    }
  __syncthreads();

  // item = (k, tile row, 8-pixel segment)
  constexpr int SEGS = TH * TW / 8;
  const int64_t OHW = (int64_t)g.OH * g.OW;
#pragma unroll
  for (int it = 0; it < KB * SEGS / 256; ++it) {
    const int idx = it * 256 + tid;
    const int seg = idx % SEGS, k = idx / SEGS;
    const int kout = k0 + k;
    const int oh = oh0 + seg / (TW / 8), ow = ow0 + (seg % (TW / 8)) * 8;
    if (kout >= g.K || oh >= g.OH || ow >= g.OW) continue;
    const i32x4 v = *(const i32x4*)(E + k * ES + seg * 8);
    unsigned short* dst =
        out + ((int64_t)n * g.K + kout) * OHW + (int64_t)oh * g.OW + ow;
    if (g.vec_out) {  // OW % 8 == 0: the segment is whole
      *(i32x4*)dst = v;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (ow + e < g.OW)
          dst[e] = (unsigned short)(((unsigned)v[e >> 1] >> ((e & 1) * 16)) &
                                    0xffff);
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------

using Kern = void (*)(const unsigned short*, const unsigned short*,
                      const float*, unsigned short*, TapGeom);

// The instantiation of a problem: the only place that decides MF and ALIGNED.
struct TapChoice {
  Kern kern;
  int mf, th, tw;
  std::string label;
};

// MF in {2, 4, 7}: the fewest padded output-channel rows, ties to the larger;
// a larger MF also wins while it costs at most K/8 more rows than the fewest,
// since every pixel fragment read from LDS is used MF times.
static int choose_mf(int K) {
  const int cand[3] = {2, 4, 7};
  int rows[3], best = INT32_MAX;
  for (int i = 0; i < 3; ++i) {
    const int kb = cand[i] * 16;
    rows[i] = (K + kb - 1) / kb * kb;
    if (rows[i] < best) best = rows[i];
  }
  for (int i = 2; i > 0; --i)
    if ((int64_t)(rows[i] - best) * 8 <= K) return cand[i];
  return cand[0];
}

template <int R, int S>
static TapChoice choose_rs(int mf, bool aligned) {
  using T = Tile<R, S>;
  const std::string label = "tap<" + std::to_string(R) + "x" +
                            std::to_string(S) + "," + std::to_string(mf) + ">";
  Kern k;
  if (mf == 2)
    k = aligned ? tap_fwd_kernel<R, S, 2, true> : tap_fwd_kernel<R, S, 2, false>;
  else if (mf == 4)
    k = aligned ? tap_fwd_kernel<R, S, 4, true> : tap_fwd_kernel<R, S, 4, false>;
  else
    k = aligned ? tap_fwd_kernel<R, S, 7, true> : tap_fwd_kernel<R, S, 7, false>;
  return {k, mf, T::TH, T::TW, label};
}

static TapChoice choose(int K, int W, int R, int S, bool base_aligned) {
  const int mf = choose_mf(K);
  const bool aligned = base_aligned && W % 8 == 0;
  if (R == 1 && S == 7) return choose_rs<1, 7>(mf, aligned);
  if (R == 7 && S == 1) return choose_rs<7, 1>(mf, aligned);
  return choose_rs<3, 3>(mf, aligned);
}

static void check_problem(int64_t N, int64_t C, int64_t K, int64_t H, int64_t W,
                          int64_t R, int64_t S, int64_t ph, int64_t pw) {
  TORCH_CHECK((R == 1 && S == 7) || (R == 7 && S == 1) || (R == 3 && S == 3),
              "tap_fwd: kernel size must be 1x7, 7x1 or 3x3 (stride 1, "
              "dilation 1, groups 1), got ", R, "x", S);
  TORCH_CHECK(N >= 1 && C >= 1 && K >= 1 && H >= 1 && W >= 1,
              "tap_fwd: N, C, K, H, W must be positive");
  TORCH_CHECK(ph >= 0 && ph <= R - 1 && pw >= 0 && pw <= S - 1,
              "tap_fwd: padding must lie in [0, R-1] x [0, S-1], got (", ph,
              ", ", pw, ") for ", R, "x", S);
  TORCH_CHECK(H + 2 * ph >= R && W + 2 * pw >= S,
              "tap_fwd: the padded input is smaller than the filter");
  TORCH_CHECK(H * W < (1LL << 30) && C < (1LL << 24) && K < (1LL << 24),
              "tap_fwd: problem too large");
}

static TapGeom make_geom(int64_t N, int64_t C, int64_t K, int64_t H, int64_t W,
                         int64_t R, int64_t S, int64_t ph, int64_t pw,
                         const TapChoice& ch) {
  TapGeom g;
  g.N = (int)N; g.C = (int)C; g.K = (int)K; g.H = (int)H; g.W = (int)W;
  g.ph = (int)ph; g.pw = (int)pw;
  g.OH = g.H + 2 * g.ph - (int)R + 1;
  g.OW = g.W + 2 * g.pw - (int)S + 1;
  g.Kp = (g.K + 15) / 16 * 16;
  g.Cp = (g.C + CK - 1) / CK * CK;
  g.row_blocks = (g.OH + ch.th - 1) / ch.th;
  g.col_blocks = (g.OW + ch.tw - 1) / ch.tw;
  g.k_tiles = (g.K + ch.mf * 16 - 1) / (ch.mf * 16);
  g.vec_out = g.OW % 8 == 0;
  return g;
}

std::string tap_kernel_name(int64_t C, int64_t K, int64_t H, int64_t W,
                            int64_t R, int64_t S, int64_t ph, int64_t pw) {
  check_problem(1, C, K, H, W, R, S, ph, pw);
  return choose((int)K, (int)W, (int)R, (int)S, true).label;
}

torch::Tensor tap_fwd(torch::Tensor x, torch::Tensor w,
                      c10::optional<torch::Tensor> bias, int64_t ph, int64_t pw,
                      bool transposed) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.get_device() == w.get_device(),
              "tap_fwd: x and w must be on one GPU");
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && x.is_contiguous() &&
                  w.is_contiguous(),
              "tap_fwd: x and w must be contiguous 4-d tensors");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
                  w.scalar_type() == torch::kBFloat16,
              "tap_fwd: bf16 only");
  const int64_t Kw = w.size(0), Cw = w.size(1), R = w.size(2), S = w.size(3);
  const int64_t Cred = transposed ? Kw : Cw, Kout = transposed ? Cw : Kw;
  check_problem(x.size(0), Cred, Kout, x.size(2), x.size(3), R, S, ph, pw);
  TORCH_CHECK(x.size(1) == Cred, "tap_fwd: channel mismatch: x has ", x.size(1),
              ", the filter reduces over ", Cred);
  const bool base_aligned = ((uintptr_t)x.data_ptr() & 15) == 0;
  const TapChoice ch =
      choose((int)Kout, (int)x.size(3), (int)R, (int)S, base_aligned);
  TapGeom g = make_geom(x.size(0), Cred, Kout, x.size(2), x.size(3), R, S, ph,
                        pw, ch);
  const float* bptr = nullptr;
  torch::Tensor b32;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->numel() == Kout,
                "tap_fwd: bias must hold one value per output channel");
    b32 = bias->to(torch::kFloat).contiguous();
    bptr = b32.data_ptr<float>();
  }
  auto out = torch::empty({g.N, g.K, g.OH, g.OW}, x.options());
  auto Wt = torch::empty({R * S, g.Kp, g.Cp}, x.options());
  g.vec_out = g.vec_out && ((uintptr_t)out.data_ptr() & 15) == 0;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int64_t fblocks = ((int64_t)g.Kp * g.Cp + 255) / 256;
  const int64_t blocks =
      (int64_t)g.k_tiles * g.row_blocks * g.col_blocks * g.N;
  TORCH_CHECK(fblocks < (1LL << 31) && blocks < (1LL << 31),
              "tap_fwd: grid too large");
  hipLaunchKernelGGL(tap_filter_kernel, dim3((uint32_t)fblocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)w.data_ptr(),
                     (unsigned short*)Wt.data_ptr(), (int)Cw, g.K, g.C, g.Kp,
                     g.Cp, (int)(R * S), transposed ? 1 : 0);
  hipLaunchKernelGGL(ch.kern, dim3((uint32_t)blocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)x.data_ptr(),
                     (const unsigned short*)Wt.data_ptr(), bptr,
                     (unsigned short*)out.data_ptr(), g);
  return out;
}

}  // namespace conv_tap

void register_conv_tap(pybind11::module_& m) {
  m.def("tap_fwd", &conv_tap::tap_fwd, pybind11::arg("x"), pybind11::arg("w"),
        pybind11::arg("bias"), pybind11::arg("ph"), pybind11::arg("pw"),
        pybind11::arg("transposed") = false,
        "tap-shift direct stride-1 conv, 1x7 / 7x1 / 3x3 (bf16 NCHW); "
        "transposed: x is the output gradient, w the forward weight, the "
        "result the data gradient");
  m.def("tap_kernel_name", &conv_tap::tap_kernel_name,
        "label of the kernel tap_fwd launches for (C, K, H, W, R, S, ph, pw); "
        "no tensor, no HIP call");
}
