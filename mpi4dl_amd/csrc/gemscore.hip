// gemscore — MI355X-native (gfx950/CDNA4) kernels for mpi4dl_amd.
//
// This translation unit holds the hand-written HIP kernels plus their
// torch bindings. Everything is written for CDNA4 directly (wave64,
// no CUDA-compat shims): see /opt/skills/guides/cdna_hip_programming.md
// for the hardware model the tiling decisions cite.
//
// Kernels:
//   * halo pack / unpack / unpack-add — one launch moves ALL strips of
//     a halo exchange between the padded tile and a flat RCCL staging
//     buffer (replaces the reference's 8 slice+clone launches,
//     /root/reference/src/torchgems/spatial.py:336-413).
//   * bn_stats — per-channel sum + centred sum-of-squares in one pass
//     (feeds TileBatchNorm2d's cross-tile reduction).
//
// Conv/pool implicit-GEMM MFMA kernels live in conv_mfma.hip.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cstdint>
#include <vector>

typedef __attribute__((ext_vector_type(8))) short s16x8_;

#define MAX_STRIPS 8
#define DEVCHECK(x) TORCH_CHECK(x, #x " failed")

namespace {

struct StripDesc {
  int64_t plane_off;  // rs * Wp + cs into a (Hp, Wp) plane
  int32_t rows;
  int32_t cols;
  int64_t buf_off;    // element offset into the flat staging buffer
};

struct StripArgs {
  StripDesc s[MAX_STRIPS];
  int32_t nstrips;
  int32_t nc;           // N*C planes
  int64_t plane_stride; // Hp*Wp
  int64_t wp;           // padded width
};

// mode: 0 = pack (tile->buf), 1 = unpack (buf->tile), 2 = unpack-add
template <typename T, int MODE>
__global__ void halo_copy_kernel(T* __restrict__ tile, T* __restrict__ buf,
                                 StripArgs a, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    int64_t rem = i;
    int si = 0;
    for (; si < a.nstrips; ++si) {  // <=8 strips: register scan
      const int64_t sz = (int64_t)a.s[si].rows * a.s[si].cols * a.nc;
      if (rem < sz) break;
      rem -= sz;
    }
    const StripDesc d = a.s[si];
    const int64_t cols = d.cols;
    const int64_t rc = (int64_t)d.rows * cols;
    const int64_t plane = rem / rc;
    const int64_t r = (rem % rc) / cols;
    const int64_t c = rem % cols;
    const int64_t tidx = plane * a.plane_stride + d.plane_off + r * a.wp + c;
    const int64_t bidx = d.buf_off + plane * rc + r * cols + c;
    if (MODE == 0)
      buf[bidx] = tile[tidx];
    else if (MODE == 1)
      tile[tidx] = buf[bidx];
    else
      tile[tidx] += buf[bidx];
  }
}

StripArgs build_args(const torch::Tensor& tile, const torch::Tensor& desc,
                     int64_t* total_out) {
  TORCH_CHECK(tile.dim() == 4, "tile must be (N,C,Hp,Wp)");
  TORCH_CHECK(desc.device().is_cpu() && desc.dtype() == torch::kInt64,
              "desc must be a CPU int64 tensor [nstrips, 4]");
  auto d = desc.accessor<int64_t, 2>();
  StripArgs a;
  a.nstrips = (int32_t)desc.size(0);
  TORCH_CHECK(a.nstrips <= MAX_STRIPS, "too many strips");
  a.nc = (int32_t)(tile.size(0) * tile.size(1));
  a.plane_stride = tile.size(2) * tile.size(3);
  a.wp = tile.size(3);
  int64_t total = 0;
  for (int i = 0; i < a.nstrips; ++i) {
    const int64_t rs = d[i][0], cs = d[i][1];
    a.s[i].rows = (int32_t)d[i][2];
    a.s[i].cols = (int32_t)d[i][3];
    a.s[i].plane_off = rs * a.wp + cs;
    a.s[i].buf_off = total;
    total += (int64_t)a.s[i].rows * a.s[i].cols * a.nc;
  }
  *total_out = total;
  return a;
}

template <int MODE>
void halo_copy(torch::Tensor tile, torch::Tensor buf, torch::Tensor desc) {
  TORCH_CHECK(tile.is_cuda() && buf.is_cuda(), "tensors must be on GPU");
  TORCH_CHECK(tile.is_contiguous() && buf.is_contiguous());
  TORCH_CHECK(tile.scalar_type() == buf.scalar_type());
  int64_t total = 0;
  StripArgs a = build_args(tile, desc, &total);
  if (total == 0) return;
  TORCH_CHECK(buf.numel() >= total, "staging buffer too small");
  const int block = 256;
  auto stream = at::cuda::getCurrentCUDAStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, tile.scalar_type(),
      "halo_copy", [&] {
        if (MODE == 2) {
          // grad strips may OVERLAP at corners (each neighbour received a
          // replicated copy of the corner in forward, so each contributes
          // a gradient): launch per strip, stream-ordered, so the adds
          // into the overlap are sequential instead of racing.
          for (int i = 0; i < a.nstrips; ++i) {
            StripArgs one;
            one.nstrips = 1;
            one.nc = a.nc;
            one.plane_stride = a.plane_stride;
            one.wp = a.wp;
            one.s[0] = a.s[i];
            const int64_t t1 = (int64_t)a.s[i].rows * a.s[i].cols * a.nc;
            one.s[0].buf_off = a.s[i].buf_off;
            const int grid1 =
                (int)std::min<int64_t>((t1 + block - 1) / block, 2048);
            hipLaunchKernelGGL((halo_copy_kernel<scalar_t, MODE>), dim3(grid1),
                               dim3(block), 0, stream.stream(),
                               tile.data_ptr<scalar_t>(),
                               buf.data_ptr<scalar_t>() + a.s[i].buf_off -
                                   one.s[0].buf_off,
                               one, t1);
          }
          return;
        }
        const int grid =
            (int)std::min<int64_t>((total + block - 1) / block, 2048);
        hipLaunchKernelGGL((halo_copy_kernel<scalar_t, MODE>), dim3(grid),
                           dim3(block), 0, stream.stream(),
                           tile.data_ptr<scalar_t>(), buf.data_ptr<scalar_t>(),
                           a, total);
      });
}

// ---------------------------------------------------------------------------
// bn_stats: per-channel sum and sum-of-squares in ONE pass over (N,C,H,W).
// One workgroup per channel-chunk; wave-level reduction then LDS combine.
// ---------------------------------------------------------------------------

template <typename T>
__global__ void bn_stats_kernel(const T* __restrict__ x, float* __restrict__ out,
                                int64_t N, int64_t C, int64_t HW) {
  // block.x = 256 threads; one block per channel; grid-stride over channels
  for (int64_t ch = blockIdx.x; ch < C; ch += gridDim.x) {
    float s = 0.f, ss = 0.f;
    for (int64_t n = 0; n < N; ++n) {
      const T* p = x + (n * C + ch) * HW;
      for (int64_t i = threadIdx.x; i < HW; i += blockDim.x) {
        const float v = (float)p[i];
        s += v;
        ss += v * v;
      }
    }
    // wave64 reduction then cross-wave via LDS
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_down(s, off, 64);
      ss += __shfl_down(ss, off, 64);
    }
    __shared__ float ls[8], lss[8];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { ls[wid] = s; lss[wid] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float ts = 0.f, tss = 0.f;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { ts += ls[w]; tss += lss[w]; }
      out[ch] = ts;
      out[C + ch] = tss;
    }
    __syncthreads();
  }
}

torch::Tensor bn_stats(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.is_contiguous());
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  auto out = torch::empty({2 * C}, x.options().dtype(torch::kFloat));
  const int grid = (int)std::min<int64_t>(C, 2048);
  auto stream = at::cuda::getCurrentCUDAStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, x.scalar_type(),
      "bn_stats", [&] {
        hipLaunchKernelGGL((bn_stats_kernel<scalar_t>), dim3(grid), dim3(256),
                           0, stream.stream(), x.data_ptr<scalar_t>(),
                           out.data_ptr<float>(), N, C, HW);
      });
  return out;
}


// ---------------------------------------------------------------------------
// Pooling (NCHW), padding-aware, global-geometry divisors.
//
// Replaces torch's eager max_pool NCHW kernels (15.5% of step time in
// profiles/r01_bench_single_gpu_kernel_stats.txt). Backward is
// gather-formulated (each input position scans the <=ceil(k/s)^2 windows
// that contain it) — no atomics.
//
// Geometry: output (oh,ow) covers input rows [oh*s-p, oh*s-p+k). For
// tile-parallel exact avg (count_include_pad=False) the divisor counts
// window cells inside the GLOBAL image: global row = gr0 + oh*s + kh
// with gr0 = tile_row_offset - p; plain case: gr0 = -p, Hg = H.
// ---------------------------------------------------------------------------

// 8 consecutive outputs per thread: the input row segment is read once
// into a register sliding window (guide G13 — vectorize ALWAYS).
template <typename T, int KK, int SS>
__global__ void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                   uint8_t* __restrict__ idx, int64_t NC,
                                   int H, int W, int OH, int OW, int k_, int s_,
                                   int p) {
  const int k = KK > 0 ? KK : k_;
  const int s = KK > 0 ? SS : s_;
  const int OW8 = (OW + 7) / 8;
  const int64_t total = NC * OH * OW8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int owc = (int)(t % OW8);
    const int oh = (int)((t / OW8) % OH);
    const int64_t plane = t / ((int64_t)OW8 * OH);
    const T* xp = x + plane * H * W;
    const int ow0 = owc * 8;
    const int h0 = oh * s - p;
    float best[8];
    uint8_t bidx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bidx[e] = 0; }
    const int w_lo = ow0 * s - p;
    for (int kh = 0; kh < (KK > 0 ? KK : k); ++kh) {
      const int h = h0 + kh;
      if (h < 0 || h >= H) continue;
      const T* row = xp + h * W;
      if (KK > 0) {
        // compile-time (k,s): span stays in registers, loops fully unroll
        constexpr int SPAN = KK > 0 ? 8 * SS + KK - SS : 1;
        float seg[SPAN];
        // 2-byte dtypes take the *_vec kernels below: explicit 16-byte vector
        // types there, because a type-generic memcpy span drops to scratch.
#pragma unroll
        for (int j = 0; j < SPAN; ++j) {
          const int w = w_lo + j;
          seg[j] = (w >= 0 && w < W) ? (float)row[w] : -INFINITY;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma unroll
          for (int kw = 0; kw < KK; ++kw) {
            const float v = seg[e * SS + kw];
            if (v > best[e]) {
              best[e] = v;
              bidx[e] = (uint8_t)(kh * KK + kw);
            }
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int wbase = w_lo + e * s;
          for (int kw = 0; kw < k; ++kw) {
            const int w = wbase + kw;
            if (w < 0 || w >= W) continue;
            const float v = (float)row[w];
            if (v > best[e]) { best[e] = v; bidx[e] = (uint8_t)(kh * k + kw); }
          }
        }
      }
    }
    const int64_t obase = plane * (int64_t)OH * OW + (int64_t)oh * OW;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ow = ow0 + e;
      if (ow < OW) { y[obase + ow] = (T)best[e]; idx[obase + ow] = bidx[e]; }
    }
  }
}

// 8 consecutive input columns per thread: the candidate output windows
// of the 8 inputs overlap, so go/idx rows are read once per (oh, thread).
// (KK, SS) compile-time specialisations fully unroll the window loops
// and fold the offset div/mod (same trick as the forward).
template <typename T, int KK, int SS>
__global__ void maxpool_bwd_kernel(const T* __restrict__ go,
                                   const uint8_t* __restrict__ idx,
                                   T* __restrict__ gi, int64_t NC, int H,
                                   int W, int OH, int OW, int k_, int s_,
                                   int p, int64_t C, int64_t go_bs) {
  const int k = KK > 0 ? KK : k_;
  const int s = KK > 0 ? SS : s_;
  const int W8 = (W + 7) / 8;
  const int64_t total = NC * H * W8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int wc = (int)(t % W8);
    const int h = (int)((t / W8) % H);
    const int64_t plane = t / ((int64_t)W8 * H);
    const int w0 = wc * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    int oh_lo = (h + p - k + 1 + s - 1) / s; if (oh_lo < 0) oh_lo = 0;
    int oh_hi = (h + p) / s; if (oh_hi > OH - 1) oh_hi = OH - 1;
    int ow_lo = (w0 + p - k + 1 + s - 1) / s; if (ow_lo < 0) ow_lo = 0;
    int ow_hi = (w0 + 7 + p) / s; if (ow_hi > OW - 1) ow_hi = OW - 1;
    // go may be a channel slice of a wider NCHW tensor (batch stride go_bs)
    const T* gop = go + (plane / C) * go_bs + (plane % C) * OH * OW;
    const uint8_t* ip = idx + plane * OH * OW;
    // at most ceil((8 + k - 1)/s) + 1 candidate columns
    constexpr int NOW = KK > 0 ? (8 + KK - 1) / SS + 1 : 0;
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
      if (KK > 0) {
#pragma unroll
        for (int j = 0; j < NOW; ++j) {
          const int ow = ow_lo + j;
          if (ow > ow_hi) break;
          const int o = oh * OW + ow;
          const int off = ip[o];
          const int r = oh * SS - p + off / KK;  // winner's input row/col
          if (r != h) continue;
          const int dw = ow * SS - p + off % KK - w0;
          const float gval = (float)gop[o];
          // acc[dw] with a RUNTIME index would force acc[] to scratch;
          // the unrolled compare keeps it in registers
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (dw == e) acc[e] += gval;
        }
      } else {
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
          const int o = oh * OW + ow;
          const int off = ip[o];
          const int r = oh * s - p + off / k;
          if (r != h) continue;
          const int dw = ow * s - p + off % k - w0;
          const float gval = (float)gop[o];
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (dw == e) acc[e] += gval;
        }
      }
    }
    const int64_t ibase = plane * (int64_t)H * W + (int64_t)h * W;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (w0 + e < W) gi[ibase + w0 + e] = (T)acc[e];
  }
}

__device__ __forceinline__ float avg_div(int oh, int ow, int s, int k,
                                         long gr0, long gc0, long Hg, long Wg,
                                         int include_pad) {
  if (include_pad) return (float)(k * k);
  long r0 = gr0 + (long)oh * s, c0 = gc0 + (long)ow * s;
  long r1 = r0 + k, c1 = c0 + k;
  if (r0 < 0) r0 = 0; if (c0 < 0) c0 = 0;
  if (r1 > Hg) r1 = Hg; if (c1 > Wg) c1 = Wg;
  long cnt = (r1 - r0) * (c1 - c0);
  return cnt > 0 ? (float)cnt : 1.f;
}

// 8 outputs per thread; compile-time (k,s) keeps the row segment in
// registers (KK=0 -> generic scalar path).
template <typename T, int KK, int SS>
__global__ void avgpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                   int64_t NC, int H, int W, int OH, int OW,
                                   int k_, int s_, int p, long gr0, long gc0,
                                   long Hg, long Wg, int include_pad) {
  const int k = KK > 0 ? KK : k_;
  const int s = KK > 0 ? SS : s_;
  const int OW8 = (OW + 7) / 8;
  const int64_t total = NC * OH * OW8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int owc = (int)(t % OW8);
    const int oh = (int)((t / OW8) % OH);
    const int64_t plane = t / ((int64_t)OW8 * OH);
    const T* xp = x + plane * H * W;
    const int ow0 = owc * 8;
    const int h0 = oh * s - p;
    const int w_lo = ow0 * s - p;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int kh = 0; kh < (KK > 0 ? KK : k); ++kh) {
      const int h = h0 + kh;
      if (h < 0 || h >= H) continue;
      const T* row = xp + h * W;
      if (KK > 0) {
        constexpr int SPAN = KK > 0 ? 8 * SS + KK - SS : 1;
        float seg[SPAN];
#pragma unroll
        for (int j = 0; j < SPAN; ++j) {
          const int w = w_lo + j;
          seg[j] = (w >= 0 && w < W) ? (float)row[w] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
          for (int kw = 0; kw < KK; ++kw) acc[e] += seg[e * SS + kw];
      } else {
        for (int e = 0; e < 8; ++e) {
          const int wb = w_lo + e * s;
          for (int kw = 0; kw < k; ++kw) {
            const int w = wb + kw;
            if (w >= 0 && w < W) acc[e] += (float)row[w];
          }
        }
      }
    }
    const int64_t obase = plane * (int64_t)OH * OW + (int64_t)oh * OW;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ow = ow0 + e;
      if (ow < OW)
        y[obase + ow] =
            (T)(acc[e] / avg_div(oh, ow, s, k, gr0, gc0, Hg, Wg, include_pad));
    }
  }
}

// 8 inputs per thread; interior windows (the overwhelming majority)
// divide by the constant k*k, skipping the per-window divisor math.
template <typename T, int KK, int SS>
__global__ void avgpool_bwd_kernel(const T* __restrict__ go, T* __restrict__ gi,
                                   int64_t NC, int H, int W, int OH, int OW,
                                   int k_, int s_, int p, long gr0, long gc0,
                                   long Hg, long Wg, int include_pad,
                                   int64_t C, int64_t go_bs) {
  const int k = KK > 0 ? KK : k_;
  const int s = KK > 0 ? SS : s_;
  const int W8 = (W + 7) / 8;
  const int64_t total = NC * H * W8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int wc = (int)(t % W8);
    const int h = (int)((t / W8) % H);
    const int64_t plane = t / ((int64_t)W8 * H);
    const int w0 = wc * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    int oh_lo = (h + p - k + 1 + s - 1) / s; if (oh_lo < 0) oh_lo = 0;
    int oh_hi = (h + p) / s; if (oh_hi > OH - 1) oh_hi = OH - 1;
    int ow_lo = (w0 + p - k + 1 + s - 1) / s; if (ow_lo < 0) ow_lo = 0;
    int ow_hi = (w0 + 7 + p) / s; if (ow_hi > OW - 1) ow_hi = OW - 1;
    const T* gop = go + (plane / C) * go_bs + (plane % C) * OH * OW;
    // interior iff every touched window lies fully inside the global image
    const bool interior =
        include_pad ||
        ((gr0 + (long)oh_lo * s) >= 0 && (gr0 + (long)oh_hi * s + k) <= Hg &&
         (gc0 + (long)ow_lo * s) >= 0 && (gc0 + (long)ow_hi * s + k) <= Wg);
    const float inv_kk = 1.f / (float)(k * k);
    if (KK == 3 && SS == 1) {
      // stride-1 k3: input w is covered by ow in [w-2+p, w+p]; compute
      // the <=10 per-row contributions once, then a 3-tap sliding sum
      // (5x fewer VALU than the predicated 8x scan)
      for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        float gd[12];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
          const int ow = ow_lo + j;
          float v = 0.f;
          if (ow <= ow_hi) {
            const float g = (float)gop[oh * OW + ow];
            v = interior ? g * inv_kk
                         : g / avg_div(oh, ow, 1, 3, gr0, gc0, Hg, Wg,
                                       include_pad);
          }
          gd[j] = v;
        }
        gd[10] = 0.f;
        gd[11] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // ow range covering input w0+e: [w0+e+p-2, w0+e+p]
          const int j0 = w0 + e + p - 2 - ow_lo;
          float sum = 0.f;
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const int j = j0 + d;
            if (j >= 0 && j < 10) sum += gd[j];
          }
          acc[e] += sum;
        }
      }
    } else {
      for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
          const float g = (float)gop[oh * OW + ow];
          const float gd =
              interior ? g * inv_kk
                       : g / avg_div(oh, ow, s, k, gr0, gc0, Hg, Wg,
                                     include_pad);
          // which of my 8 inputs does window (oh, ow) cover?
          const int wlo = ow * s - p;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int w = w0 + e;
            if (w >= wlo && w < wlo + k && w < W) acc[e] += gd;
          }
        }
      }
    }
    const int64_t ibase = plane * (int64_t)H * W + (int64_t)h * W;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (w0 + e < W) gi[ibase + w0 + e] = (T)acc[e];
  }
}

// ---------------------------------------------------------------------------
// Vectorised pooling for 2-byte dtypes (bf16 / fp16).
//
// Host-side predicate (pool_vec_ok): W % 8 == 0, OW % 8 == 0, 16-byte
// aligned bases, geometry (k,s,p) in {(3,1,1), (3,2,1), (2,2,0)}. Each
// thread owns one 16-byte column chunk and walks a strip of POOL_R rows
// with a sliding register window, so every row is loaded once per thread
// with one 16-byte load (+ one narrow neighbour load per side, an L1 hit).
// Only the first/last chunk of a row and out-of-plane rows are predicated.
//
// Results are bit-identical to the generic kernels above: the same scan
// order and strict '>' for max (so the same u8 index), the same fp32
// summation order and divisions for avg. Adding +0.f for a padded tap
// equals skipping it because no accumulator here can hold -0.f.
// ---------------------------------------------------------------------------

constexpr int POOL_R = 4;  // rows per strip

template <typename T>
__device__ __forceinline__ void ld8f(const T* __restrict__ p, float* f) {
  const s16x8_ v = *(const s16x8_*)p;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (float)((const T*)&v)[e];
}

template <typename T>
__device__ __forceinline__ void st8f(T* __restrict__ p, const float* f) {
  s16x8_ v;
#pragma unroll
  for (int e = 0; e < 8; ++e) ((T*)&v)[e] = (T)f[e];
  *(s16x8_*)p = v;
}

__device__ __forceinline__ void ld8idx(const uint8_t* __restrict__ p, int* o) {
  const uint2 v = *(const uint2*)p;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] = (int)((v.x >> (8 * e)) & 255u);
    o[4 + e] = (int)((v.y >> (8 * e)) & 255u);
  }
}

__device__ __forceinline__ void st8idx(uint8_t* __restrict__ p, const int* o) {
  uint2 v;
  v.x = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) |
        ((uint32_t)o[3] << 24);
  v.y = (uint32_t)o[4] | ((uint32_t)o[5] << 8) | ((uint32_t)o[6] << 16) |
        ((uint32_t)o[7] << 24);
  *(uint2*)p = v;
}

// Row maxima of a 3-wide window for 8 outputs: m[e] / kw[e] are the first
// maximum of input row h over columns (8c+e)*S-1 .. +2 (strict '>' from
// -inf, kw 0 when nothing beats -inf). xc points at column 8*S*c of the
// plane. Out-of-plane rows give (-inf, 0), which never wins downstream.
template <typename T, int S>
__device__ __forceinline__ void max3_row(const T* __restrict__ xc, int h, int H,
                                         int W, bool hasl, bool hasr, float* m,
                                         int* kw) {
  constexpr int SPAN = 8 * S + 3 - S;  // 10 (s=1) or 17 (s=2)
  float seg[SPAN];
  if (h < 0 || h >= H) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { m[e] = -INFINITY; kw[e] = 0; }
    return;
  }
  const T* row = xc + (int64_t)h * W;
  seg[0] = hasl ? (float)row[-1] : -INFINITY;
  ld8f(row, seg + 1);
  if (S == 2) ld8f(row + 8, seg + 9);
  else seg[9] = hasr ? (float)row[8] : -INFINITY;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float b = -INFINITY;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = seg[e * S + j];
      if (v > b) { b = v; bi = j; }
    }
    m[e] = b;
    kw[e] = bi;
  }
}

// max pool k3 p1, stride S in {1,2}. Scanning the three row maxima in kh
// order with strict '>' picks the first maximum in kh-major, kw-minor
// order, exactly like the generic scan.
template <typename T, int S>
__global__ void __launch_bounds__(256)
maxpool3_fwd_vec(const T* __restrict__ x, T* __restrict__ y,
                 uint8_t* __restrict__ idx, int64_t NC, int H, int W, int OH,
                 int OW) {
  const int CH = OW >> 3;
  const int NS = (OH + POOL_R - 1) / POOL_R;
  const int64_t total = NC * NS * CH;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int c = (int)(t % CH);
    const int64_t q = t / CH;
    const int oh0 = (int)(q % NS) * POOL_R;
    const int64_t plane = q / NS;
    const T* xc = x + plane * H * W + c * 8 * S;
    const int64_t ob = plane * OH * OW + c * 8;
    const bool hasl = c > 0, hasr = c < CH - 1;
    float ma[8], mb[8], mc[8];
    int ka[8], kb[8], kc[8];
    max3_row<T, S>(xc, oh0 * S - 1, H, W, hasl, hasr, ma, ka);
    if (S == 1) max3_row<T, S>(xc, oh0, H, W, hasl, hasr, mb, kb);
#pragma unroll
    for (int r = 0; r < POOL_R; ++r) {
      const int oh = oh0 + r;
      if (oh >= OH) break;
      if (S == 2) max3_row<T, S>(xc, oh * 2, H, W, hasl, hasr, mb, kb);
      max3_row<T, S>(xc, oh * S + 1, H, W, hasl, hasr, mc, kc);
      float best[8];
      int bi[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float b = -INFINITY;
        int i = 0;
        if (ma[e] > b) { b = ma[e]; i = ka[e]; }
        if (mb[e] > b) { b = mb[e]; i = 3 + kb[e]; }
        if (mc[e] > b) { b = mc[e]; i = 6 + kc[e]; }
        best[e] = b;
        bi[e] = i;
      }
      st8f(y + ob + (int64_t)oh * OW, best);
      st8idx(idx + ob + (int64_t)oh * OW, bi);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (S == 1) { ma[e] = mb[e]; ka[e] = kb[e]; mb[e] = mc[e]; kb[e] = kc[e]; }
        else { ma[e] = mc[e]; ka[e] = kc[e]; }
      }
    }
  }
}

// max pool k2 s2 p0: 16 input columns -> 8 outputs, no padding anywhere.
template <typename T>
__global__ void __launch_bounds__(256)
maxpool2s2_fwd_vec(const T* __restrict__ x, T* __restrict__ y,
                   uint8_t* __restrict__ idx, int64_t NC, int H, int W, int OH,
                   int OW) {
  const int CH = OW >> 3;
  const int NS = (OH + POOL_R - 1) / POOL_R;
  const int64_t total = NC * NS * CH;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int c = (int)(t % CH);
    const int64_t q = t / CH;
    const int oh0 = (int)(q % NS) * POOL_R;
    const int64_t plane = q / NS;
    const T* xc = x + plane * H * W + c * 16;
    const int64_t ob = plane * OH * OW + c * 8;
#pragma unroll
    for (int r = 0; r < POOL_R; ++r) {
      const int oh = oh0 + r;
      if (oh >= OH) break;
      float s0[16], s1[16];
      const T* row = xc + (int64_t)(oh * 2) * W;
      ld8f(row, s0);
      ld8f(row + 8, s0 + 8);
      ld8f(row + W, s1);
      ld8f(row + W + 8, s1 + 8);
      float best[8];
      int bi[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float b = -INFINITY;
        int i = 0;
        if (s0[2 * e] > b) { b = s0[2 * e]; i = 0; }
        if (s0[2 * e + 1] > b) { b = s0[2 * e + 1]; i = 1; }
        if (s1[2 * e] > b) { b = s1[2 * e]; i = 2; }
        if (s1[2 * e + 1] > b) { b = s1[2 * e + 1]; i = 3; }
        best[e] = b;
        bi[e] = i;
      }
      st8f(y + ob + (int64_t)oh * OW, best);
      st8idx(idx + ob + (int64_t)oh * OW, bi);
    }
  }
}

// One row of (go, idx) candidates for a backward thread: NJ = 10 covers
// ow = 8c-1 .. 8c+8 (stride 1), NJ = 9 covers ow = 8c .. 8c+8 (k3 s2).
// Invalid candidates get g = 0 and the impossible window offset 255.
template <typename T, int NJ>
__device__ __forceinline__ void go_row(const T* __restrict__ gc,
                                       const uint8_t* __restrict__ ic, int oh,
                                       int OH, int OW, bool hasl, bool hasr,
                                       float* g, int* o) {
  constexpr int L = NJ - 9;  // 1 when a left neighbour is needed
  if (oh < 0 || oh >= OH) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) { g[j] = 0.f; o[j] = 255; }
    return;
  }
  const T* gr = gc + (int64_t)oh * OW;
  const uint8_t* ir = ic + (int64_t)oh * OW;
  ld8f(gr, g + L);
  ld8idx(ir, o + L);
  if (L == 1) {
    g[0] = hasl ? (float)gr[-1] : 0.f;
    o[0] = hasl ? (int)ir[-1] : 255;
  }
  g[L + 8] = hasr ? (float)gr[8] : 0.f;
  o[L + 8] = hasr ? (int)ir[8] : 255;
}

// max pool backward k3 s1 p1. Input (h, 8c+e) gathers from go rows
// h-1, h, h+1 (kh = 2, 1, 0) and columns ow = 8c+e-1 .. +1 (kw = 2, 1, 0),
// added in ascending (oh, ow) order like the generic kernel.
template <typename T>
__global__ void __launch_bounds__(256)
maxpool3s1_bwd_vec(const T* __restrict__ go, const uint8_t* __restrict__ idx,
                   T* __restrict__ gi, int64_t NC, int H, int W, int64_t C,
                   int64_t go_bs) {
  const int CH = W >> 3;
  const int NS = (H + POOL_R - 1) / POOL_R;
  const int64_t total = NC * NS * CH;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int c = (int)(t % CH);
    const int64_t q = t / CH;
    const int h0 = (int)(q % NS) * POOL_R;
    const int64_t plane = q / NS;
    const int64_t HW = (int64_t)H * W;
    const T* gc = go + (plane / C) * go_bs + (plane % C) * HW + c * 8;
    const uint8_t* ic = idx + plane * HW + c * 8;
    T* gic = gi + plane * HW + c * 8;
    const bool hasl = c > 0, hasr = c < CH - 1;
    float g0[10], g1[10], g2[10];
    int o0[10], o1[10], o2[10];
    go_row<T, 10>(gc, ic, h0 - 1, H, W, hasl, hasr, g0, o0);
    go_row<T, 10>(gc, ic, h0, H, W, hasl, hasr, g1, o1);
#pragma unroll
    for (int r = 0; r < POOL_R; ++r) {
      const int h = h0 + r;
      if (h >= H) break;
      go_row<T, 10>(gc, ic, h + 1, H, W, hasl, hasr, g2, o2);
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) a += (o0[e + j] == 6 + 2 - j) ? g0[e + j] : 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) a += (o1[e + j] == 3 + 2 - j) ? g1[e + j] : 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) a += (o2[e + j] == 2 - j) ? g2[e + j] : 0.f;
        acc[e] = a;
      }
      st8f(gic + (int64_t)h * W, acc);
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        g0[j] = g1[j]; o0[j] = o1[j];
        g1[j] = g2[j]; o1[j] = o2[j];
      }
    }
  }
}

// max pool backward k3 s2 p1: 16 input columns <- 9 candidate outputs per
// go row. Input rows come in pairs: row 2q gathers from go row q (kh = 1),
// row 2q+1 from go row q (kh = 2) then q+1 (kh = 0). Even columns 2m see
// (ow = 8c+m, kw = 1); odd columns 2m+1 see (m, kw = 2) then (m+1, kw = 0).
template <typename T>
__global__ void __launch_bounds__(256)
maxpool3s2_bwd_vec(const T* __restrict__ go, const uint8_t* __restrict__ idx,
                   T* __restrict__ gi, int64_t NC, int H, int W, int OH, int OW,
                   int64_t C, int64_t go_bs) {
  const int CH = OW >> 3;  // == W / 16
  const int NP = (H + 1) >> 1;  // input row pairs (== OH)
  const int NS = (NP + POOL_R - 1) / POOL_R;
  const int64_t total = NC * NS * CH;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int c = (int)(t % CH);
    const int64_t q = t / CH;
    const int p0 = (int)(q % NS) * POOL_R;
    const int64_t plane = q / NS;
    const int64_t OHW = (int64_t)OH * OW;
    const T* gc = go + (plane / C) * go_bs + (plane % C) * OHW + c * 8;
    const uint8_t* ic = idx + plane * OHW + c * 8;
    T* gic = gi + plane * (int64_t)H * W + c * 16;
    const bool hasr = c < CH - 1;
    float ga[9], gb[9];
    int oa[9], ob[9];
    go_row<T, 9>(gc, ic, p0, OH, OW, false, hasr, ga, oa);
#pragma unroll
    for (int r = 0; r < POOL_R; ++r) {
      const int pr = p0 + r;
      if (pr >= NP) break;
      go_row<T, 9>(gc, ic, pr + 1, OH, OW, false, hasr, gb, ob);
      float acc[16];
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        float a = 0.f;
        a += (oa[m] == 4) ? ga[m] : 0.f;
        acc[2 * m] = a;
        float b = 0.f;
        b += (oa[m] == 5) ? ga[m] : 0.f;
        b += (oa[m + 1] == 3) ? ga[m + 1] : 0.f;
        acc[2 * m + 1] = b;
      }
      T* row = gic + (int64_t)(2 * pr) * W;
      st8f(row, acc);
      st8f(row + 8, acc + 8);
      if (2 * pr + 1 < H) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          float a = 0.f;
          a += (oa[m] == 7) ? ga[m] : 0.f;
          a += (ob[m] == 1) ? gb[m] : 0.f;
          acc[2 * m] = a;
          float b = 0.f;
          b += (oa[m] == 8) ? ga[m] : 0.f;
          b += (oa[m + 1] == 6) ? ga[m + 1] : 0.f;
          b += (ob[m] == 2) ? gb[m] : 0.f;
          b += (ob[m + 1] == 0) ? gb[m + 1] : 0.f;
          acc[2 * m + 1] = b;
        }
        st8f(row + W, acc);
        st8f(row + W + 8, acc + 8);
      }
#pragma unroll
      for (int j = 0; j < 9; ++j) { ga[j] = gb[j]; oa[j] = ob[j]; }
    }
  }
}

// max pool backward k2 s2 p0: input (h, w) has the single candidate
// (h/2, w/2), window offset (h%2)*2 + w%2. An odd last row has none.
template <typename T>
__global__ void __launch_bounds__(256)
maxpool2s2_bwd_vec(const T* __restrict__ go, const uint8_t* __restrict__ idx,
                   T* __restrict__ gi, int64_t NC, int H, int W, int OH, int OW,
                   int64_t C, int64_t go_bs) {
  const int CH = OW >> 3;  // == W / 16
  const int NP = (H + 1) >> 1;
  const int NS = (NP + POOL_R - 1) / POOL_R;
  const int64_t total = NC * NS * CH;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int c = (int)(t % CH);
    const int64_t q = t / CH;
    const int p0 = (int)(q % NS) * POOL_R;
    const int64_t plane = q / NS;
    const int64_t OHW = (int64_t)OH * OW;
    const T* gc = go + (plane / C) * go_bs + (plane % C) * OHW + c * 8;
    const uint8_t* ic = idx + plane * OHW + c * 8;
    T* gic = gi + plane * (int64_t)H * W + c * 16;
#pragma unroll
    for (int r = 0; r < POOL_R; ++r) {
      const int pr = p0 + r;
      if (pr >= NP) break;
      float g[8];
      int o[8];
      if (pr < OH) {
        ld8f(gc + (int64_t)pr * OW, g);
        ld8idx(ic + (int64_t)pr * OW, o);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { g[e] = 0.f; o[e] = 255; }
      }
      T* row = gic + (int64_t)(2 * pr) * W;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        if (2 * pr + kh >= H) break;
        float acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float a = 0.f;
          a += (o[e >> 1] == kh * 2 + (e & 1)) ? g[e >> 1] : 0.f;
          acc[e] = a;
        }
        st8f(row + (int64_t)kh * W, acc);
        st8f(row + (int64_t)kh * W + 8, acc + 8);
      }
    }
  }
}

// One input row of avg pool k3 s1 p1 taps: columns 8c-1 .. 8c+8, zeros
// for padding.
template <typename T>
__device__ __forceinline__ void avg_row(const T* __restrict__ xc, int h, int H,
                                        int W, bool hasl, bool hasr,
                                        float* seg) {
  if (h < 0 || h >= H) {
#pragma unroll
    for (int j = 0; j < 10; ++j) seg[j] = 0.f;
    return;
  }
  const T* row = xc + (int64_t)h * W;
  seg[0] = hasl ? (float)row[-1] : 0.f;
  ld8f(row, seg + 1);
  seg[9] = hasr ? (float)row[8] : 0.f;
}

// avg pool k3 s1 p1: nine taps per output summed kh-major, kw-minor in
// fp32, one division by the generic kernel's avg_div.
template <typename T>
__global__ void __launch_bounds__(256)
avgpool3s1_fwd_vec(const T* __restrict__ x, T* __restrict__ y, int64_t NC,
                   int H, int W, long gr0, long gc0, long Hg, long Wg,
                   int include_pad) {
  const int CH = W >> 3;
  const int NS = (H + POOL_R - 1) / POOL_R;
  const int64_t total = NC * NS * CH;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int c = (int)(t % CH);
    const int64_t q = t / CH;
    const int oh0 = (int)(q % NS) * POOL_R;
    const int64_t plane = q / NS;
    const T* xc = x + plane * H * W + c * 8;
    T* yc = y + plane * H * W + c * 8;
    const bool hasl = c > 0, hasr = c < CH - 1;
    // every window of this chunk lies inside the global image column-wise
    const bool col_in = (gc0 + c * 8) >= 0 && (gc0 + c * 8 + 7 + 3) <= Wg;
    float s0[10], s1[10], s2[10];
    avg_row<T>(xc, oh0 - 1, H, W, hasl, hasr, s0);
    avg_row<T>(xc, oh0, H, W, hasl, hasr, s1);
#pragma unroll
    for (int r = 0; r < POOL_R; ++r) {
      const int oh = oh0 + r;
      if (oh >= H) break;
      avg_row<T>(xc, oh + 1, H, W, hasl, hasr, s2);
      float dv[8];
      if (include_pad || (col_in && (gr0 + oh) >= 0 && (gr0 + oh + 3) <= Hg)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) dv[e] = 9.f;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          dv[e] = avg_div(oh, c * 8 + e, 1, 3, gr0, gc0, Hg, Wg, 0);
      }
      float out[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) a += s0[e + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) a += s1[e + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) a += s2[e + j];
        out[e] = a / dv[e];
      }
      st8f(yc + (int64_t)oh * W, out);
#pragma unroll
      for (int j = 0; j < 10; ++j) { s0[j] = s1[j]; s1[j] = s2[j]; }
    }
  }
}

// One go row for the avg backward in both scalings the generic kernel
// can apply: gm = g * (1/9) (what an interior thread uses) and, only when
// this strip has a non-interior thread-row (need_div), gd = g / avg_div.
template <typename T>
__device__ __forceinline__ void avg_go_row(const T* __restrict__ gc, int oh,
                                           int H, int W, int c, bool hasl,
                                           bool hasr, bool need_div, long gr0,
                                           long gc0, long Hg, long Wg,
                                           float* gm, float* gd) {
  float g[10];
  avg_row<T>(gc, oh, H, W, hasl, hasr, g);
  const float inv_kk = 1.f / 9.f;
#pragma unroll
  for (int j = 0; j < 10; ++j) { gm[j] = g[j] * inv_kk; gd[j] = 0.f; }
  if (need_div && oh >= 0 && oh < H) {
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int ow = c * 8 - 1 + j;
      if (ow >= 0 && ow < W)
        gd[j] = g[j] / avg_div(oh, ow, 1, 3, gr0, gc0, Hg, Wg, 0);
    }
  }
}

// avg pool backward k3 s1 p1. Keeps the generic <3,1> arithmetic: per go
// row a three-tap `sum` in ascending ow, then acc += sum in ascending oh;
// the scaling is g * (1/9) when the thread-row is interior (judged on the
// same clipped candidate ranges) and g / avg_div otherwise.
template <typename T>
__global__ void __launch_bounds__(256)
avgpool3s1_bwd_vec(const T* __restrict__ go, T* __restrict__ gi, int64_t NC,
                   int H, int W, long gr0, long gc0, long Hg, long Wg,
                   int include_pad, int64_t C, int64_t go_bs) {
  const int CH = W >> 3;
  const int NS = (H + POOL_R - 1) / POOL_R;
  const int64_t total = NC * NS * CH;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int c = (int)(t % CH);
    const int64_t q = t / CH;
    const int h0 = (int)(q % NS) * POOL_R;
    const int64_t plane = q / NS;
    const int64_t HW = (int64_t)H * W;
    const T* gc = go + (plane / C) * go_bs + (plane % C) * HW + c * 8;
    T* gic = gi + plane * HW + c * 8;
    const bool hasl = c > 0, hasr = c < CH - 1;
    const int ow_lo = hasl ? c * 8 - 1 : 0;
    const int ow_hi = hasr ? c * 8 + 8 : W - 1;
    const bool col_in = (gc0 + ow_lo) >= 0 && (gc0 + ow_hi + 3) <= Wg;
    // rows h0-1 .. h0+R clipped to the plane bound every candidate range
    // of this strip; if they are all inside the image no thread-row of the
    // strip needs the division
    const int r_lo = h0 > 0 ? h0 - 1 : 0;
    const int r_hi = h0 + POOL_R < H ? h0 + POOL_R : H - 1;
    const bool need_div =
        !include_pad &&
        !(col_in && (gr0 + r_lo) >= 0 && (gr0 + r_hi + 3) <= Hg);
    float m0[10], m1[10], m2[10], d0[10], d1[10], d2[10];
    avg_go_row<T>(gc, h0 - 1, H, W, c, hasl, hasr, need_div, gr0, gc0, Hg, Wg,
                  m0, d0);
    avg_go_row<T>(gc, h0, H, W, c, hasl, hasr, need_div, gr0, gc0, Hg, Wg, m1,
                  d1);
#pragma unroll
    for (int r = 0; r < POOL_R; ++r) {
      const int h = h0 + r;
      if (h >= H) break;
      avg_go_row<T>(gc, h + 1, H, W, c, hasl, hasr, need_div, gr0, gc0, Hg, Wg,
                    m2, d2);
      const int oh_lo = h > 0 ? h - 1 : 0;
      const int oh_hi = h + 1 < H ? h + 1 : H - 1;
      const bool interior =
          include_pad ||
          (col_in && (gr0 + oh_lo) >= 0 && (gr0 + oh_hi + 3) <= Hg);
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float a = 0.f;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) s += interior ? m0[e + j] : d0[e + j];
        a += s;
        s = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) s += interior ? m1[e + j] : d1[e + j];
        a += s;
        s = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) s += interior ? m2[e + j] : d2[e + j];
        a += s;
        acc[e] = a;
      }
      st8f(gic + (int64_t)h * W, acc);
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        m0[j] = m1[j]; d0[j] = d1[j];
        m1[j] = m2[j]; d1[j] = d2[j];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Fused BatchNorm (NCHW), one kernel family for every plane shape:
// fp64-accumulated channel stats, one normalize+affine(+ReLU) pass,
// gather-formulated backward. Replaces MIOpenBatchNorm{Fwd,Bwd}Spatial
// and the surrounding unfused elementwise casts; doubles as the
// local-stats leg of TileBatchNorm2d's cross-tile sync (python does one
// allreduce of the [sum,sumsq] / [gsum,gxsum] vectors between the two
// kernels). Statistics may be restricted to a region = rows
// [top, H-bottom) x cols [left, W-right) of every plane (surplus tiles
// of the D2 fused-halo design are e.g. 259x259 with a margin).
//
// All kernels walk 16-byte SLOTS of the flat tensor (the tensor base is
// 16-byte aligned — enforced host-side), so every vector access is
// aligned whatever the row / plane start is. The reductions load a whole
// slot wherever it lies inside the tensor and mask the elements outside
// their range (head and tail of a row or plane); the elementwise kernels
// resolve a slot that straddles a plane seam per element. Both give every
// element the same arithmetic whichever way its slot was resolved, so
// results do not depend on where the planes fall on the slot grid.
//
// WHOLE (apply, backward statistics, backward apply): the host saw that
// every access is a whole in-bounds slot — HW is a multiple of VEC — so
// the element masks, the bounds test and the per-element branch compile
// out; the body is otherwise the same. Measured on the benchmark
// (profiles/PERF_NOTES.md): without it these kernels are up to 4 % slower
// on whole-slot planes than the aligned kernels they replaced. The
// full-plane statistics stayed slower even so, and keep their aligned
// kernel (bn_stats64_kernel) on the same predicate.
// ---------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ float to_f32(T v) { return (float)v; }

// [sum, sumsq] of the elements of slot [v0, v0+VEC) that lie in [a, e).
template <typename T>
__device__ __forceinline__ void stats_slot(const T* __restrict__ x, int64_t v0,
                                           int64_t a, int64_t e, int64_t numel,
                                           double& s, double& ss) {
  constexpr int VEC = 16 / sizeof(T);
  const int lo = (int)max(a - v0, (int64_t)0);
  const int hi = (int)min(e - v0, (int64_t)VEC);
  if (v0 + VEC <= numel) {
    const uint4 raw = *(const uint4*)(x + v0);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float f = to_f32(((const T*)&raw)[k]);
      f = (k >= lo && k < hi) ? f : 0.f;
      s += (double)f;
      ss += (double)(f * f);
    }
  } else {
    for (int k = lo; k < hi; ++k) {
      const float f = to_f32(x[v0 + k]);
      s += (double)f;
      ss += (double)(f * f);
    }
  }
}

// block-wide sum of (s, ss) into out[ch], out[C + ch]: one fp64 atomicAdd
// per block per output
__device__ __forceinline__ void stats_block_commit(double s, double ss,
                                                   double* __restrict__ out,
                                                   int64_t C, int64_t ch) {
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    ss += __shfl_down(ss, off, 64);
  }
  __shared__ double ls[8], lss[8];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { ls[wid] = s; lss[wid] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = 0.0, tss = 0.0;
    for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) { ts += ls[wv]; tss += lss[wv]; }
    atomicAdd(&out[ch], ts);
    atomicAdd(&out[C + ch], tss);
  }
}

// j / d for j * d < 2^32 with m = 2^32 / d + 1 (host-checked)
__device__ __forceinline__ uint32_t fast_div(uint32_t j, uint32_t d,
                                             uint32_t m) {
  return d == 1 ? j : __umulhi(j, m);
}

// Contiguous range [start, start+total) of every plane: the whole plane,
// or a region whose rows are full width. 2D grid: x = channel, y = chunk
// (the chip needs >>256 workgroups); the chunk windows start at the plane
// range's first SLOT, so every block walks chunk/VEC whole slots whatever
// the plane's alignment.
template <typename T>
__global__ void bn_stats64_span_kernel(const T* __restrict__ x,
                                       double* __restrict__ out, int64_t N,
                                       int64_t C, int64_t HW, int64_t start,
                                       int64_t total, int64_t chunk) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t ch = blockIdx.x;
  const int64_t numel = N * C * HW;
  double s = 0.0, ss = 0.0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t a0 = (n * C + ch) * HW + start;
    const int64_t w0 = a0 / VEC * VEC + (int64_t)blockIdx.y * chunk;
    const int64_t a = max(a0, w0);
    const int64_t e = min(a0 + total, w0 + chunk);
    for (int64_t v0 = w0 + (int64_t)threadIdx.x * VEC; v0 < e;
         v0 += (int64_t)blockDim.x * VEC)
      stats_slot<T>(x, v0, a, e, numel, s, ss);
  }
  stats_block_commit(s, ss, out, C, ch);
}

// The whole plane when every plane is made of whole slots (HW % VEC == 0,
// aligned base): chunk windows are plain element ranges of the plane and
// nothing is masked. Kept beside the span kernel because the span kernel,
// even with its masks compiled out, measured 1.1-1.7 % slower on the
// benchmark's planes (profiles/PERF_NOTES.md).
template <typename T>
__global__ void bn_stats64_kernel(const T* __restrict__ x,
                                  double* __restrict__ out, int64_t N,
                                  int64_t C, int64_t HW, int64_t chunk) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t ch = blockIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * chunk;
  const int64_t i1 = min(i0 + chunk, HW);
  double s = 0.0, ss = 0.0;
  for (int64_t n = 0; n < N; ++n) {
    const T* p = x + (n * C + ch) * HW;
    for (int64_t i = i0 + (int64_t)threadIdx.x * VEC; i + VEC <= i1;
         i += (int64_t)blockDim.x * VEC) {
      const uint4 raw = *(const uint4*)(p + i);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float f = to_f32(((const T*)&raw)[k]);
        s += (double)f;
        ss += (double)(f * f);
      }
    }
  }
  stats_block_commit(s, ss, out, C, ch);
}

// Region with a left/right margin: rows of `len` elements, `W` apart,
// the first `start` into each plane. 2D grid: x = channel, y = block of
// `rpc` rows; the (image, row, slot) triples of a block are dealt to its
// threads as one flat index.
template <typename T>
__global__ void bn_stats64_region_kernel(const T* __restrict__ x,
                                         double* __restrict__ out, int64_t N,
                                         int64_t C, int64_t HW, int64_t start,
                                         int len, int W, int nrows, int rpc,
                                         uint32_t S, uint32_t mS) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t ch = blockIdx.x;
  const int64_t numel = N * C * HW;
  const int r0 = (int)blockIdx.y * rpc;
  const uint32_t rows = (uint32_t)(min(r0 + rpc, nrows) - r0);
  const uint32_t mR = (uint32_t)(((uint64_t)1 << 32) / rows + 1);
  const uint32_t work = (uint32_t)N * rows * S;
  double s = 0.0, ss = 0.0;
  for (uint32_t j = threadIdx.x; j < work; j += blockDim.x) {
    const uint32_t q = fast_div(j, S, mS);     // image * rows + row
    const uint32_t sl = j - q * S;             // slot within the row
    const uint32_t n = fast_div(q, rows, mR);
    const uint32_t r = q - n * rows;
    const int64_t a =
        ((int64_t)n * C + ch) * HW + start + (int64_t)(r0 + (int)r) * W;
    const int64_t e = a + len;
    const int64_t v0 = (a / VEC + sl) * VEC;
    if (v0 < e) stats_slot<T>(x, v0, a, e, numel, s, ss);
  }
  stats_block_commit(s, ss, out, C, ch);
}

// y = (x - mean) * invstd * w + b (+ ReLU). A slot inside one plane takes
// its channel once; a slot across a plane seam or the flat tail goes per
// element.
template <typename T, bool RELU, bool WHOLE>
__global__ void bn_apply_kernel(const T* __restrict__ x, T* __restrict__ y,
                                const float* __restrict__ mean,
                                const float* __restrict__ invstd,
                                const float* __restrict__ wgt,
                                const float* __restrict__ bias, int64_t total,
                                int64_t C, int64_t HW) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t nvec = (total + VEC - 1) / VEC;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t iv = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iv < nvec;
       iv += stride) {
    const int64_t i = iv * VEC;
    const int64_t p0 = i / HW;
    if (WHOLE || (i + VEC <= total && i - p0 * HW + VEC <= HW)) {
      const int64_t ch = p0 % C;
      const float m = mean[ch], inv = invstd[ch], w = wgt[ch], b = bias[ch];
      const uint4 rx = *(const uint4*)(x + i);
      uint4 ry;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float v = (to_f32(((const T*)&rx)[e]) - m) * inv * w + b;
        if (RELU) v = v > 0.f ? v : 0.f;
        ((T*)&ry)[e] = (T)v;
      }
      *(uint4*)(y + i) = ry;
    } else {
      const int64_t k1 = min(i + VEC, total);
      for (int64_t k = i; k < k1; ++k) {
        const int64_t ch = (k / HW) % C;
        float v = (to_f32(x[k]) - mean[ch]) * invstd[ch] * wgt[ch] + bias[ch];
        if (RELU) v = v > 0.f ? v : 0.f;
        y[k] = (T)v;
      }
    }
  }
}

// per-channel [gsum, gxsum] where gxsum = sum(go * xhat); RELU masks go
// by (y > 0) — pass y=nullptr when no fusion. Block (ch, y) sums one chunk
// of every image's plane; chunk windows start at the plane's first slot
// (see bn_stats64_span_kernel), elements outside the plane are masked.
template <typename T, bool RELU, bool WHOLE>
__global__ void bn_bwd_stats_kernel(const T* __restrict__ go,
                                    const T* __restrict__ x,
                                    const T* __restrict__ y,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ invstd,
                                    double* __restrict__ out, int64_t N,
                                    int64_t C, int64_t HW, int64_t chunk) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t ch = blockIdx.x;
  const int64_t numel = N * C * HW;
  const float m = mean[ch], inv = invstd[ch];
  double gs = 0.0, gx = 0.0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t a0 = (n * C + ch) * HW;
    const int64_t w0 = a0 / VEC * VEC + (int64_t)blockIdx.y * chunk;
    const int64_t a = max(a0, w0);
    const int64_t e = min(a0 + HW, w0 + chunk);
    for (int64_t v0 = w0 + (int64_t)threadIdx.x * VEC; v0 < e;
         v0 += (int64_t)blockDim.x * VEC) {
      const int lo = WHOLE ? 0 : (int)max(a - v0, (int64_t)0);
      const int hi = WHOLE ? VEC : (int)min(e - v0, (int64_t)VEC);
      if (WHOLE || v0 + VEC <= numel) {
        const uint4 rg = *(const uint4*)(go + v0);
        const uint4 rx = *(const uint4*)(x + v0);
        uint4 ry;
        if (RELU) ry = *(const uint4*)(y + v0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          float g = to_f32(((const T*)&rg)[k]);
          if (RELU && to_f32(((const T*)&ry)[k]) <= 0.f) g = 0.f;
          const float xh = (to_f32(((const T*)&rx)[k]) - m) * inv;
          const bool in = k >= lo && k < hi;
          gs += (double)(in ? g : 0.f);
          gx += (double)(in ? g * xh : 0.f);
        }
      } else {
        for (int k = lo; k < hi; ++k) {
          float g = to_f32(go[v0 + k]);
          if (RELU && to_f32(y[v0 + k]) <= 0.f) g = 0.f;
          const float xh = (to_f32(x[v0 + k]) - m) * inv;
          gs += (double)g;
          gx += (double)(g * xh);
        }
      }
    }
  }
  stats_block_commit(gs, gx, out, C, ch);
}

// gi of one element; `reduced` = the two reduction terms reach this pixel
__device__ __forceinline__ float bn_bwd_elem(float g, float xh, float gsn,
                                             float gxn, float w, float inv,
                                             bool reduced) {
  return (reduced ? g - gsn - xh * gxn : g) * w * inv;
}

// a reduction term sum/n from the fp64 statistic: the statistic is rounded
// to fp32 first, which is what the fp32 cast of the statistics followed by
// (float)(sum * inv_n) gave
__device__ __forceinline__ float bn_bwd_term(double st, double inv_n) {
  return (float)((double)(float)st * inv_n);
}

// gi = w*inv*(g - gsum/n - xhat*gxsum/n). gsum/gxsum are the (group-wide)
// fp64 statistics. With `local` (the tile's own fp64 [gsum, gxsum]) block 0
// also produces the parameter gradients gb = (float)local[:C], gw =
// (float)local[C:]: added in place into gb_acc / gw_acc where given, else
// written to pgrad[2C]. REGION: mean/var came from the
// region pixels only while every pixel was normalised, so the two
// reduction terms reach region pixels only:
//   gi_p = w*inv*[g_p - 1{p in region}*(gsum/n + xhat_p*gxsum/n)]
template <typename T, bool RELU, bool REGION, bool WHOLE>
__global__ void bn_bwd_apply_kernel(
    const T* __restrict__ go, const T* __restrict__ x, const T* __restrict__ y,
    T* __restrict__ gi, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ wgt,
    const double* __restrict__ gsum, const double* __restrict__ gxsum,
    const double* __restrict__ local, float* __restrict__ gw_acc,
    float* __restrict__ gb_acc, float* __restrict__ pgrad, double inv_n,
    int64_t total, int64_t C, int64_t HW, int W, int row_lo, int row_hi,
    int col_lo, int col_hi) {
  constexpr int VEC = 16 / sizeof(T);
  if (blockIdx.x == 0 && local != nullptr) {
    // parameter gradients, one owner per element: the fp32 cast of the
    // local sums, added into the gradient buffer or written to pgrad[2C]
    for (int64_t ch = threadIdx.x; ch < C; ch += blockDim.x) {
      const float b = (float)local[ch], w = (float)local[C + ch];
      if (gb_acc != nullptr) gb_acc[ch] += b; else pgrad[ch] = b;
      if (gw_acc != nullptr) gw_acc[ch] += w; else pgrad[C + ch] = w;
    }
  }
  const int64_t nvec = (total + VEC - 1) / VEC;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t iv = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iv < nvec;
       iv += stride) {
    const int64_t i = iv * VEC;
    const int64_t p0 = i / HW;
    const int64_t rem = i - p0 * HW;
    if (WHOLE || (i + VEC <= total && rem + VEC <= HW)) {
      const int64_t ch = p0 % C;
      const float m = mean[ch], inv = invstd[ch], w = wgt[ch];
      const float gsn = bn_bwd_term(gsum[ch], inv_n);
      const float gxn = bn_bwd_term(gxsum[ch], inv_n);
      int row = 0, col = 0;
      if (REGION) {
        row = (int)(rem / W);
        col = (int)(rem - (int64_t)row * W);
      }
      const uint4 rg = *(const uint4*)(go + i);
      const uint4 rx = *(const uint4*)(x + i);
      uint4 ry;
      if (RELU) ry = *(const uint4*)(y + i);
      uint4 ro;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float g = to_f32(((const T*)&rg)[e]);
        if (RELU && to_f32(((const T*)&ry)[e]) <= 0.f) g = 0.f;
        const float xh = (to_f32(((const T*)&rx)[e]) - m) * inv;
        bool reduced = true;
        if (REGION) {
          reduced = row >= row_lo && row < row_hi && col >= col_lo &&
                    col < col_hi;
          if (++col == W) { col = 0; ++row; }
        }
        ((T*)&ro)[e] = (T)bn_bwd_elem(g, xh, gsn, gxn, w, inv, reduced);
      }
      *(uint4*)(gi + i) = ro;
    } else {
      const int64_t k1 = min(i + VEC, total);
      for (int64_t k = i; k < k1; ++k) {
        const int64_t p = k / HW;
        const int64_t ch = p % C;
        const float inv = invstd[ch];
        float g = to_f32(go[k]);
        if (RELU && to_f32(y[k]) <= 0.f) g = 0.f;
        const float xh = (to_f32(x[k]) - mean[ch]) * inv;
        bool reduced = true;
        if (REGION) {
          const int64_t q = k - p * HW;
          const int row = (int)(q / W);
          const int col = (int)(q - (int64_t)row * W);
          reduced = row >= row_lo && row < row_hi && col >= col_lo &&
                    col < col_hi;
        }
        gi[k] = (T)bn_bwd_elem(g, xh, bn_bwd_term(gsum[ch], inv_n),
                               bn_bwd_term(gxsum[ch], inv_n), wgt[ch], inv,
                               reduced);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// State fan backward (ops/fuse.py, state_fan): the gradient of a cell
// state y that was handed to several consumers, some through relu(y).
// One pass reads every consumer's gradient once and writes
//
//   m = select(r <= 0, 0, fold(rel[0], rel[1], ...))          r = relu(y)
//   g = fold(raw[0], ..., raw[slot-1], m, raw[slot], ...)
//
// where fold is a LEFT fold whose every partial sum is rounded to T: that
// is what a chain of torch adds on T tensors (autograd's accumulation of
// one gradient after the other) produces, so g has the same bits as the
// unfused chain when the caller passes the terms in the order autograd
// would have met them.
//
// Every term is dense or a channel slice of a contiguous NCHW tensor:
// dense planes and channels, its own batch stride. r and g are dense.
// Grid: y = image, x walks the image's C*HW elements V at a time; V is a
// 16-byte slot when HW is a multiple of it and every base is aligned,
// else 1. Pointers and strides travel by value in the kernel arguments.
// ---------------------------------------------------------------------------

constexpr int FAN_MAX = 4;  // raw terms, and ReLU terms, at most

struct FanTerms {
  const void* raw[FAN_MAX];
  const void* rel[FAN_MAX];
  int64_t raw_bs[FAN_MAX];
  int64_t rel_bs[FAN_MAX];
};

template <typename T, int V>
struct alignas(sizeof(T) * V) FanPack {
  T v[V];
};

template <typename T, int NRAW, int NREL, int V>
__global__ void __launch_bounds__(256)
    fan_bwd_kernel(const FanTerms t, const T* __restrict__ r,
                   T* __restrict__ g, int64_t per_img, int slot) {
  using acc_t = std::conditional_t<std::is_same<T, double>::value, double, float>;
  using Pack = FanPack<T, V>;
  const int64_t n = blockIdx.y;
  const int64_t nv = per_img / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t iv = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iv < nv;
       iv += stride) {
    const int64_t i = iv * V;
    Pack raw[NRAW ? NRAW : 1], rel[NREL ? NREL : 1], rr, out;
#pragma unroll
    for (int k = 0; k < NRAW; ++k)
      raw[k] = *(const Pack*)((const T*)t.raw[k] + n * t.raw_bs[k] + i);
#pragma unroll
    for (int k = 0; k < NREL; ++k)
      rel[k] = *(const Pack*)((const T*)t.rel[k] + n * t.rel_bs[k] + i);
    if (NREL) rr = *(const Pack*)(r + n * per_img + i);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      // a fold's first term enters as it is; a + b == b + a, so the masked
      // sum in slot 0 may be added to raw[0] instead of the other way round
      acc_t m = (acc_t)0;
      if (NREL) {
        m = (acc_t)rel[0].v[e];
#pragma unroll
        for (int k = 1; k < NREL; ++k)
          m = (acc_t)(T)(m + (acc_t)rel[k].v[e]);
        if ((acc_t)rr.v[e] <= (acc_t)0) m = (acc_t)0;
      }
      acc_t a = m;
      if (NRAW) {
        a = (acc_t)raw[0].v[e];
        if (NREL && slot == 0) a = (acc_t)(T)(a + m);
#pragma unroll
        for (int k = 1; k <= NRAW; ++k) {
          if (NREL && k == slot) a = (acc_t)(T)(a + m);
          if (k < NRAW) a = (acc_t)(T)(a + (acc_t)raw[k].v[e]);
        }
      }
      out.v[e] = (T)a;
    }
    *(Pack*)(g + n * per_img + i) = out;
  }
}

// ---------------------------------------------------------------------------
// Fused momentum-SGD on flat fp32 buffers: one kernel for the whole
// model step (replaces ~3 torch launches per parameter — the profile
// showed 5.8k tiny CUDAFunctor_add kernels per step).
//   v = mu*v + g (+ wd*p);  p -= lr*v;  then g = 0.
// ---------------------------------------------------------------------------

__global__ void sgd_momentum_kernel(float* __restrict__ p,
                                    float* __restrict__ g,
                                    float* __restrict__ v, float lr, float mu,
                                    float wd, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 pv = *(float4*)(p + i * 4);
    float4 gv = *(float4*)(g + i * 4);
    float4 vv = *(float4*)(v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float grad = ((float*)&gv)[e] + wd * ((float*)&pv)[e];
      float vel = mu * ((float*)&vv)[e] + grad;
      ((float*)&vv)[e] = vel;
      ((float*)&pv)[e] = ((float*)&pv)[e] - lr * vel;
      ((float*)&gv)[e] = 0.f;
    }
    *(float4*)(p + i * 4) = pv;
    *(float4*)(v + i * 4) = vv;
    *(float4*)(g + i * 4) = gv;
  }
}

void sgd_momentum(torch::Tensor p, torch::Tensor g, torch::Tensor v,
                  double lr, double mu, double wd) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() && g.is_contiguous() &&
              v.is_contiguous());
  TORCH_CHECK(p.scalar_type() == torch::kFloat);
  TORCH_CHECK(p.numel() % 4 == 0, "flat buffer must be padded to 4");
  const int64_t n4 = p.numel() / 4;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int grid = (int)std::min<int64_t>((n4 + 255) / 256, 2048);
  hipLaunchKernelGGL(sgd_momentum_kernel, dim3(grid), dim3(256), 0,
                     stream.stream(), p.data_ptr<float>(),
                     g.data_ptr<float>(), v.data_ptr<float>(), (float)lr,
                     (float)mu, (float)wd, n4);
}

// bn_finalize: fold the fp64 [sum,sumsq] -> [mean, invstd] conversion,
// the running-stat EMA update and num_batches_tracked into ONE kernel
// (the python glue cost ~8 small launches per BN call). `zero2`, when
// given, is a second fp64 [2C] vector that is zero-filled on the way: the
// accumulator of this forward's bn_bwd_stats.
__global__ void bn_finalize_kernel(double* __restrict__ stats,
                                   float* __restrict__ out,
                                   float* __restrict__ rmean,
                                   float* __restrict__ rvar,
                                   int64_t* __restrict__ tracked, float mom,
                                   double n, float eps, int64_t C,
                                   int rezero, double* __restrict__ zero2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C) return;
  if (zero2) {            // the backward statistics' accumulator of this
    zero2[i] = 0.0;       // forward (bn_bwd_stats out): zeroed here, so the
    zero2[C + i] = 0.0;   // backward launches no fill
  }
  const double mean = stats[i] / n;
  double var = stats[C + i] / n - mean * mean;
  if (var < 0.0) var = 0.0;
  if (rezero) {
    stats[i] = 0.0;       // restore the zero invariant for the next
    stats[C + i] = 0.0;   // bn_stats64_acc accumulation (no fill kernel)
  }
  out[i] = (float)mean;
  out[C + i] = rsqrtf((float)var + eps);
  if (rmean) {
    rmean[i] = (1.f - mom) * rmean[i] + mom * (float)mean;
    const float unb = (float)(var * (n / (n > 1.0 ? n - 1.0 : 1.0)));
    rvar[i] = (1.f - mom) * rvar[i] + mom * unb;
  }
  if (i == 0 && tracked) tracked[0] += 1;
}

torch::Tensor bn_finalize(torch::Tensor stats,
                          c10::optional<torch::Tensor> rmean,
                          c10::optional<torch::Tensor> rvar,
                          c10::optional<torch::Tensor> tracked, double mom,
                          double n, double eps, bool rezero = false,
                          c10::optional<torch::Tensor> zero2 = c10::nullopt) {
  const int64_t C = stats.numel() / 2;
  if (zero2.has_value())
    TORCH_CHECK(zero2->is_cuda() && zero2->is_contiguous() &&
                    zero2->scalar_type() == torch::kDouble &&
                    zero2->numel() == 2 * C &&
                    zero2->get_device() == stats.get_device(),
                "bn_finalize: zero2 must be a contiguous fp64 CUDA vector of "
                "2*C on stats' device");
  auto out = torch::empty({2 * C}, stats.options().dtype(torch::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(
      bn_finalize_kernel, dim3((uint32_t)((C + 255) / 256)), dim3(256), 0,
      stream.stream(), stats.data_ptr<double>(), out.data_ptr<float>(),
      rmean.has_value() ? rmean->data_ptr<float>() : nullptr,
      rvar.has_value() ? rvar->data_ptr<float>() : nullptr,
      tracked.has_value() ? tracked->data_ptr<int64_t>() : nullptr,
      (float)mom, n, (float)eps, C, rezero ? 1 : 0,
      zero2.has_value() ? zero2->data_ptr<double>() : nullptr);
  return out;
}


// ---------------- torch-facing wrappers ----------------

static inline int grid_for(int64_t total, int block) {
  int64_t g = (total + block - 1) / block;
  return (int)std::min<int64_t>(g, 4096);
}

// grid for the *_vec pool kernels: one thread per (plane, strip, chunk)
static inline int pool_vec_grid(int64_t threads) {
  return (int)std::min<int64_t>((threads + 255) / 256, 1 << 20);
}

static inline int64_t pool_strips(int64_t rows) {
  return (rows + POOL_R - 1) / POOL_R;
}

static inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// Shape half of the fast-path predicate: 2-byte dtype, whole 16-byte
// chunks on both sides, and (H, W) <-> (OH, OW) consistent with (k,s,p).
static bool pool_vec_shape_ok(int64_t itemsize, int64_t H, int64_t W,
                              int64_t OH, int64_t OW, int64_t k, int64_t s,
                              int64_t p) {
  const bool geom = (k == 3 && s == 1 && p == 1) ||
                    (k == 3 && s == 2 && p == 1) ||
                    (k == 2 && s == 2 && p == 0);
  if (!geom) return false;
  if (itemsize != 2) return false;  // Half and BFloat16
  if (H < 1 || W < 8 || OH < 1 || OW < 8 || W % 8 != 0 || OW % 8 != 0)
    return false;
  if (OH != (H + 2 * p - k) / s + 1 || OW != (W + 2 * p - k) / s + 1)
    return false;
  if (s == 2 && W != 2 * OW) return false;
  return H * W < (int64_t(1) << 30);
}

// A 4-D gradient that is a channel slice of a contiguous NCHW tensor:
// dense planes, dense channels, free batch stride.
static bool go_plane_dense(const torch::Tensor& go) {
  return go.dim() == 4 && go.stride(3) == 1 && go.stride(2) == go.size(3) &&
         go.stride(1) == go.size(2) * go.size(3) && go.stride(0) >= 0;
}

// Launchers for the *_vec kernels; only 2-byte dtypes instantiate them
// (the host predicate never selects them for anything else).
template <typename T>
void maxpool_fwd_vec(const T* x, T* y, uint8_t* idx, int64_t NC, int H, int W,
                     int OH, int OW, int k, int s, hipStream_t stream) {
  if constexpr (sizeof(T) == 2) {
    const dim3 grid(pool_vec_grid(NC * pool_strips(OH) * (OW / 8)));
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, x, y, idx, NC, H,
                         W, OH, OW);
    };
    if (k == 2) launch(maxpool2s2_fwd_vec<T>);
    else if (s == 1) launch(maxpool3_fwd_vec<T, 1>);
    else launch(maxpool3_fwd_vec<T, 2>);
  } else {
    TORCH_CHECK(false, "pool fast path needs a 2-byte dtype");
  }
}

template <typename T>
void maxpool_bwd_vec(const T* go, const uint8_t* idx, T* gi, int64_t NC, int H,
                     int W, int OH, int OW, int k, int s, int64_t C,
                     int64_t go_bs, hipStream_t stream) {
  if constexpr (sizeof(T) == 2) {
    const int64_t chunks = s == 1 ? W / 8 : W / 16;
    const int64_t rows = s == 1 ? H : (H + 1) / 2;
    const dim3 grid(pool_vec_grid(NC * pool_strips(rows) * chunks));
    if (s == 1) {
      hipLaunchKernelGGL(maxpool3s1_bwd_vec<T>, grid, dim3(256), 0, stream, go,
                         idx, gi, NC, H, W, C, go_bs);
    } else {
      auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, go, idx, gi, NC,
                           H, W, OH, OW, C, go_bs);
      };
      if (k == 3) launch(maxpool3s2_bwd_vec<T>);
      else launch(maxpool2s2_bwd_vec<T>);
    }
  } else {
    TORCH_CHECK(false, "pool fast path needs a 2-byte dtype");
  }
}

template <typename T>
void avgpool_fwd_vec(const T* x, T* y, int64_t NC, int H, int W, int64_t gr0,
                     int64_t gc0, int64_t Hg, int64_t Wg, bool include_pad,
                     hipStream_t stream) {
  if constexpr (sizeof(T) == 2) {
    const dim3 grid(pool_vec_grid(NC * pool_strips(H) * (W / 8)));
    hipLaunchKernelGGL(avgpool3s1_fwd_vec<T>, grid, dim3(256), 0, stream, x, y,
                       NC, H, W, (long)gr0, (long)gc0, (long)Hg, (long)Wg,
                       include_pad ? 1 : 0);
  } else {
    TORCH_CHECK(false, "pool fast path needs a 2-byte dtype");
  }
}

template <typename T>
void avgpool_bwd_vec(const T* go, T* gi, int64_t NC, int H, int W, int64_t gr0,
                     int64_t gc0, int64_t Hg, int64_t Wg, bool include_pad,
                     int64_t C, int64_t go_bs, hipStream_t stream) {
  if constexpr (sizeof(T) == 2) {
    const dim3 grid(pool_vec_grid(NC * pool_strips(H) * (W / 8)));
    hipLaunchKernelGGL(avgpool3s1_bwd_vec<T>, grid, dim3(256), 0, stream, go,
                       gi, NC, H, W, (long)gr0, (long)gc0, (long)Hg, (long)Wg,
                       include_pad ? 1 : 0, C, go_bs);
  } else {
    TORCH_CHECK(false, "pool fast path needs a 2-byte dtype");
  }
}

// ---------------- pool kernel choice ----------------
// One chooser for the four bindings and for pool_kernel_name: the label
// is spelt from the same (vec, kk, ss) the launch switches on.

enum class PoolOp { MaxFwd, MaxBwd, AvgFwd, AvgBwd };

struct PoolChoice {
  bool vec;   // a *_vec kernel for (kk, ss); else <kk, ss> of the generic one
  int kk, ss; // generic: the template arguments, <0,0> = runtime (k, s)
  std::string label;
};

static inline int64_t pool_out(int64_t n, int64_t k, int64_t s, int64_t p) {
  return (n + 2 * p - k) / s + 1;
}

// `aligned`: the tensors are non-empty and every base pointer of the
// launch is 16-byte aligned. `go_bs`: batch stride of go in elements for
// the backward ops (0 = contiguous).
static PoolChoice choose_pool(PoolOp op, int64_t itemsize, int64_t H,
                              int64_t W, int64_t k, int64_t s, int64_t p,
                              bool aligned, int64_t go_bs,
                              bool force_generic) {
  const bool is_max = op == PoolOp::MaxFwd || op == PoolOp::MaxBwd;
  const bool is_bwd = op == PoolOp::MaxBwd || op == PoolOp::AvgBwd;
  const bool vec =
      !force_generic && aligned && (is_max || (k == 3 && s == 1)) &&
      pool_vec_shape_ok(itemsize, H, W, pool_out(H, k, s, p),
                        pool_out(W, k, s, p), k, s, p) &&
      (!is_bwd || go_bs % 8 == 0);
  PoolChoice c{vec, (int)k, (int)s, ""};
  const std::string dir = is_bwd ? "_bwd" : "_fwd";
  if (vec) {
    if (!is_max)
      c.label = "vec:avg3s1" + dir;
    else if (k == 3 && !is_bwd)
      c.label = "vec:max3_fwd<" + std::to_string(c.ss) + ">";
    else
      c.label = "vec:max" + std::to_string(c.kk) + "s" + std::to_string(c.ss) +
                dir;
    return c;
  }
  const bool spec = (k == 3 && (s == 1 || s == 2)) ||
                    (is_max && k == 2 && s == 2);
  if (!spec) c.kk = c.ss = 0;
  c.label = std::string(is_max ? "max" : "avg") + dir + "<" +
            std::to_string(c.kk) + "," + std::to_string(c.ss) + ">";
  return c;
}

// Geometry every pool binding needs before it sizes anything.
static void check_pool_geom(const char* who, int64_t H, int64_t W, int64_t k,
                            int64_t s, int64_t p) {
  TORCH_CHECK(k >= 1, who, ": kernel size must be >= 1, got k=", k);
  TORCH_CHECK(s >= 1, who, ": stride must be >= 1, got s=", s);
  TORCH_CHECK(p >= 0, who, ": padding must be >= 0, got p=", p);
  TORCH_CHECK(2 * p <= k, who, ": padding must be at most half the kernel, "
              "got p=", p, " k=", k);
  TORCH_CHECK(H + 2 * p >= k && W + 2 * p >= k, who, ": kernel larger than "
              "the padded input, got H=", H, " W=", W, " k=", k, " p=", p);
}

static void check_pool_out(const char* who, const torch::Tensor& t,
                           const char* what, int64_t H, int64_t W, int64_t k,
                           int64_t s, int64_t p) {
  TORCH_CHECK(t.dim() == 4, who, ": ", what, " must be 4-D");
  const int64_t OH = pool_out(H, k, s, p), OW = pool_out(W, k, s, p);
  TORCH_CHECK(t.size(2) == OH && t.size(3) == OW, who, ": ", what, " is ",
              t.size(2), "x", t.size(3), " but (H, W, k, s, p) give ", OH, "x",
              OW);
}

std::string pool_kernel_name(const std::string& op, int64_t itemsize, int64_t H,
                             int64_t W, int64_t k, int64_t s, int64_t p,
                             bool aligned, int64_t go_bs) {
  check_pool_geom("pool_kernel_name", H, W, k, s, p);
  PoolOp o;
  if (op == "max_fwd") o = PoolOp::MaxFwd;
  else if (op == "max_bwd") o = PoolOp::MaxBwd;
  else if (op == "avg_fwd") o = PoolOp::AvgFwd;
  else if (op == "avg_bwd") o = PoolOp::AvgBwd;
  else TORCH_CHECK(false, "pool_kernel_name: op must be max_fwd, max_bwd, "
                   "avg_fwd or avg_bwd, got ", op);
  return choose_pool(o, itemsize, H, W, k, s, p, aligned, go_bs, false).label;
}

std::vector<torch::Tensor> maxpool_fwd(torch::Tensor x, int64_t k, int64_t s,
                                       int64_t p, bool force_generic) {
  TORCH_CHECK(x.dim() == 4, "maxpool_fwd: x must be 4-D");
  check_pool_geom("maxpool_fwd", x.size(2), x.size(3), k, s, p);
  TORCH_CHECK(k * k <= 256,
              "maxpool_fwd: k*k must fit the u8 window index, got k=", k);
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  const int64_t N = x.size(0), C = x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  const int OH = (H + 2 * (int)p - (int)k) / (int)s + 1;
  const int OW = (W + 2 * (int)p - (int)k) / (int)s + 1;
  auto y = torch::empty({N, C, OH, OW}, x.options());
  auto idx = torch::empty({N, C, OH, OW}, x.options().dtype(torch::kByte));
  const int64_t total = N * C * (int64_t)OH * OW;
  auto stream = at::cuda::getCurrentCUDAStream();
  const PoolChoice ch = choose_pool(
      PoolOp::MaxFwd, x.element_size(), H, W, k, s, p,
      total > 0 && aligned16(x.data_ptr()) && aligned16(y.data_ptr()) &&
          aligned16(idx.data_ptr()),
      0, force_generic);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, x.scalar_type(),
      "maxpool_fwd", [&] {
        if (ch.vec) {
          maxpool_fwd_vec<scalar_t>(x.data_ptr<scalar_t>(),
                                    y.data_ptr<scalar_t>(),
                                    idx.data_ptr<uint8_t>(), N * C, H, W, OH, OW,
                                    ch.kk, ch.ss, stream.stream());
          return;
        }
        auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, dim3(grid_for(total, 256)), dim3(256), 0,
                             stream.stream(), x.data_ptr<scalar_t>(),
                             y.data_ptr<scalar_t>(), idx.data_ptr<uint8_t>(),
                             N * C, H, W, OH, OW, (int)k, (int)s, (int)p);
        };
        if (ch.kk == 3 && ch.ss == 2)
          launch(maxpool_fwd_kernel<scalar_t, 3, 2>);
        else if (ch.kk == 3 && ch.ss == 1)
          launch(maxpool_fwd_kernel<scalar_t, 3, 1>);
        else if (ch.kk == 2 && ch.ss == 2)
          launch(maxpool_fwd_kernel<scalar_t, 2, 2>);
        else if (ch.kk == 0)
          launch(maxpool_fwd_kernel<scalar_t, 0, 0>);
        else
          TORCH_CHECK(false, "maxpool_fwd: no kernel for ", ch.label);
      });
  return {y, idx};
}

torch::Tensor maxpool_bwd(torch::Tensor go, torch::Tensor idx, int64_t H,
                          int64_t W, int64_t k, int64_t s, int64_t p,
                          bool force_generic) {
  check_pool_geom("maxpool_bwd", H, W, k, s, p);
  check_pool_out("maxpool_bwd", go, "go", H, W, k, s, p);
  check_pool_out("maxpool_bwd", idx, "idx", H, W, k, s, p);
  TORCH_CHECK(idx.size(0) == go.size(0) && idx.size(1) == go.size(1),
              "maxpool_bwd: idx and go disagree on (N, C)");
  TORCH_CHECK(k * k <= 256,
              "maxpool_bwd: k*k must fit the u8 window index, got k=", k);
  const bool go_contig = go.is_contiguous();
  TORCH_CHECK(go.is_cuda() && (go_contig || go_plane_dense(go)),
              "maxpool_bwd: go must be a channel slice of a contiguous NCHW "
              "tensor");
  TORCH_CHECK(idx.is_cuda() && idx.is_contiguous() &&
              idx.scalar_type() == torch::kByte && idx.numel() == go.numel());
  const int64_t N = go.size(0), C = go.size(1);
  const int OH = (int)go.size(2), OW = (int)go.size(3);
  const int64_t go_bs = go_contig ? C * OH * OW : go.stride(0);
  auto gi = torch::empty({N, C, H, W}, go.options());
  const int64_t total = N * C * H * W;
  auto stream = at::cuda::getCurrentCUDAStream();
  const PoolChoice ch = choose_pool(
      PoolOp::MaxBwd, go.element_size(), H, W, k, s, p,
      total > 0 && go.numel() > 0 && aligned16(go.data_ptr()) &&
          aligned16(idx.data_ptr()) && aligned16(gi.data_ptr()),
      go_bs, force_generic);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, go.scalar_type(),
      "maxpool_bwd", [&] {
        if (ch.vec) {
          maxpool_bwd_vec<scalar_t>(go.data_ptr<scalar_t>(),
                                    idx.data_ptr<uint8_t>(),
                                    gi.data_ptr<scalar_t>(), N * C, (int)H,
                                    (int)W, OH, OW, ch.kk, ch.ss, C, go_bs,
                                    stream.stream());
          return;
        }
        auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, dim3(grid_for(total, 256)), dim3(256), 0,
                             stream.stream(), go.data_ptr<scalar_t>(),
                             idx.data_ptr<uint8_t>(), gi.data_ptr<scalar_t>(),
                             N * C, (int)H, (int)W, OH, OW, (int)k, (int)s,
                             (int)p, C, go_bs);
        };
        if (ch.kk == 3 && ch.ss == 1)
          launch(maxpool_bwd_kernel<scalar_t, 3, 1>);
        else if (ch.kk == 3 && ch.ss == 2)
          launch(maxpool_bwd_kernel<scalar_t, 3, 2>);
        else if (ch.kk == 2 && ch.ss == 2)
          launch(maxpool_bwd_kernel<scalar_t, 2, 2>);
        else if (ch.kk == 0)
          launch(maxpool_bwd_kernel<scalar_t, 0, 0>);
        else
          TORCH_CHECK(false, "maxpool_bwd: no kernel for ", ch.label);
      });
  return gi;
}

torch::Tensor avgpool_fwd(torch::Tensor x, int64_t k, int64_t s, int64_t p,
                          int64_t gr0, int64_t gc0, int64_t Hg, int64_t Wg,
                          bool include_pad, bool force_generic) {
  TORCH_CHECK(x.dim() == 4, "avgpool_fwd: x must be 4-D");
  check_pool_geom("avgpool_fwd", x.size(2), x.size(3), k, s, p);
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  const int64_t N = x.size(0), C = x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  const int OH = (H + 2 * (int)p - (int)k) / (int)s + 1;
  const int OW = (W + 2 * (int)p - (int)k) / (int)s + 1;
  auto y = torch::empty({N, C, OH, OW}, x.options());
  const int64_t total = N * C * (int64_t)OH * OW;
  auto stream = at::cuda::getCurrentCUDAStream();
  const PoolChoice ch = choose_pool(
      PoolOp::AvgFwd, x.element_size(), H, W, k, s, p,
      total > 0 && aligned16(x.data_ptr()) && aligned16(y.data_ptr()), 0,
      force_generic);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, x.scalar_type(),
      "avgpool_fwd", [&] {
        if (ch.vec) {
          avgpool_fwd_vec<scalar_t>(x.data_ptr<scalar_t>(),
                                    y.data_ptr<scalar_t>(), N * C, H, W, gr0,
                                    gc0, Hg, Wg, include_pad, stream.stream());
          return;
        }
        auto launch = [&](auto kern) {
          hipLaunchKernelGGL(kern, dim3(grid_for(total, 256)), dim3(256), 0,
                             stream.stream(), x.data_ptr<scalar_t>(),
                             y.data_ptr<scalar_t>(), N * C, H, W, OH, OW,
                             (int)k, (int)s, (int)p, (long)gr0, (long)gc0,
                             (long)Hg, (long)Wg, include_pad ? 1 : 0);
        };
        if (ch.kk == 3 && ch.ss == 2)
          launch(avgpool_fwd_kernel<scalar_t, 3, 2>);
        else if (ch.kk == 3 && ch.ss == 1)
          launch(avgpool_fwd_kernel<scalar_t, 3, 1>);
        else if (ch.kk == 0)
          launch(avgpool_fwd_kernel<scalar_t, 0, 0>);
        else
          TORCH_CHECK(false, "avgpool_fwd: no kernel for ", ch.label);
      });
  return y;
}

torch::Tensor avgpool_bwd(torch::Tensor go, int64_t H, int64_t W, int64_t k,
                          int64_t s, int64_t p, int64_t gr0, int64_t gc0,
                          int64_t Hg, int64_t Wg, bool include_pad,
                          bool force_generic) {
  check_pool_geom("avgpool_bwd", H, W, k, s, p);
  check_pool_out("avgpool_bwd", go, "go", H, W, k, s, p);
  const bool go_contig = go.is_contiguous();
  TORCH_CHECK(go.is_cuda() && (go_contig || go_plane_dense(go)),
              "avgpool_bwd: go must be a channel slice of a contiguous NCHW "
              "tensor");
  const int64_t N = go.size(0), C = go.size(1);
  const int OH = (int)go.size(2), OW = (int)go.size(3);
  const int64_t go_bs = go_contig ? C * OH * OW : go.stride(0);
  auto gi = torch::empty({N, C, H, W}, go.options());
  const int64_t total = N * C * H * W;
  auto stream = at::cuda::getCurrentCUDAStream();
  const PoolChoice ch = choose_pool(
      PoolOp::AvgBwd, go.element_size(), H, W, k, s, p,
      total > 0 && go.numel() > 0 && aligned16(go.data_ptr()) &&
          aligned16(gi.data_ptr()),
      go_bs, force_generic);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, go.scalar_type(),
      "avgpool_bwd", [&] {
        if (ch.vec) {
          avgpool_bwd_vec<scalar_t>(go.data_ptr<scalar_t>(),
                                    gi.data_ptr<scalar_t>(), N * C, (int)H,
                                    (int)W, gr0, gc0, Hg, Wg, include_pad, C,
                                    go_bs, stream.stream());
          return;
        }
        auto launch = [&](auto kern) {
          hipLaunchKernelGGL(kern, dim3(grid_for(total, 256)), dim3(256), 0,
                             stream.stream(), go.data_ptr<scalar_t>(),
                             gi.data_ptr<scalar_t>(), N * C, (int)H, (int)W,
                             OH, OW, (int)k, (int)s, (int)p, (long)gr0,
                             (long)gc0, (long)Hg, (long)Wg,
                             include_pad ? 1 : 0, C, go_bs);
        };
        if (ch.kk == 3 && ch.ss == 2)
          launch(avgpool_bwd_kernel<scalar_t, 3, 2>);
        else if (ch.kk == 3 && ch.ss == 1)
          launch(avgpool_bwd_kernel<scalar_t, 3, 1>);
        else if (ch.kk == 0)
          launch(avgpool_bwd_kernel<scalar_t, 0, 0>);
        else
          TORCH_CHECK(false, "avgpool_bwd: no kernel for ", ch.label);
      });
  return gi;
}

// ---------------- BatchNorm bindings ----------------
// Every binding checks its arguments first, for every shape: x is a
// contiguous 4-D CUDA tensor, go / y are laid out like x, the per-channel
// vectors are fp32 of length C. A base off the 16-byte grid is cloned.

static void check_bn_x(const torch::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.is_contiguous(),
              "bn: x must be a contiguous 4-D CUDA tensor");
}

static void check_bn_like(const torch::Tensor& t, const torch::Tensor& x,
                          const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.sizes() == x.sizes() &&
                  t.scalar_type() == x.scalar_type(),
              "bn: ", name, " must be contiguous with x's shape and dtype");
}

static void check_bn_vec(const torch::Tensor& v, int64_t C, const char* name) {
  TORCH_CHECK(v.is_cuda() && v.scalar_type() == torch::kFloat &&
                  v.is_contiguous() && v.numel() == C,
              "bn: ", name, " must be a contiguous fp32 CUDA vector of ", C,
              " channels");
}

static void check_bn_out(const torch::Tensor& out, int64_t C) {
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
                  out.scalar_type() == torch::kDouble && out.numel() == 2 * C,
              "bn: out must be a contiguous fp64 CUDA vector of 2*C");
}

static void check_margin(const std::vector<int64_t>& mg, int64_t H,
                         int64_t W) {
  TORCH_CHECK(mg.size() == 4, "margin is (top, bottom, left, right)");
  TORCH_CHECK(mg[0] >= 0 && mg[1] >= 0 && mg[2] >= 0 && mg[3] >= 0 &&
                  mg[0] + mg[1] < H && mg[2] + mg[3] < W,
              "margin leaves an empty region of a ", H, "x", W, " plane");
}

// the BN kernels take 16-byte slots of the flat tensor from its base
static torch::Tensor slot_aligned(const torch::Tensor& t) {
  return aligned16(t.data_ptr()) ? t : t.clone();
}

// f(std::true_type / std::false_type) for a run-time bool: one launch site
// serves every instantiation of a kernel's bool template parameters
template <typename F>
static void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// (chunk, gy) of a stats grid that sums `span` elements of every plane:
// ~2048 workgroups (256 CUs x 8) over C channels, chunk a multiple of
// 2048. A chunk window starts at the first slot of the plane's range, up
// to `slack` elements before the range itself.
static std::pair<int64_t, int64_t> stats_grid(int64_t C, int64_t HW,
                                              int64_t span, int64_t slack) {
  const int64_t splits =
      std::min(std::max<int64_t>(1, 2048 / std::max<int64_t>(C, 1)),
               std::max<int64_t>(1, (HW + 2047) / 2048));
  const int64_t chunk = ((HW + splits - 1) / splits + 2047) / 2048 * 2048;
  return {chunk, (span + slack + chunk - 1) / chunk};
}

// slack of a range that starts `start` into every plane of an aligned
// tensor: none when all of them start on a slot boundary
static int64_t slot_slack(int64_t vec, int64_t HW, int64_t start) {
  return (HW % vec == 0 && start % vec == 0) ? 0 : vec - 1;
}

// WHOLE of the kernels: every plane of an aligned tensor is made of whole
// in-bounds slots
static bool planes_whole(int64_t vec, int64_t HW) { return HW % vec == 0; }

// Accumulate [sum, sumsq] of the region (margin = top, bottom, left,
// right) into a caller-owned ZEROED fp64 buffer (persistent across steps;
// bn_finalize(..., rezero=true) restores the invariant) — kills the
// per-BN-call torch.zeros fill kernel (~3k launches/step).
torch::Tensor bn_stats64_region_acc(torch::Tensor x, torch::Tensor out,
                                    std::vector<int64_t> margin) {
  check_bn_x(x);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t HW = H * W;
  check_margin(margin, H, W);
  check_bn_out(out, C);
  const int64_t mt = margin[0], mb = margin[1], ml = margin[2], mr = margin[3];
  x = slot_aligned(x);
  const int64_t Hr = H - mt - mb;
  const int64_t vec = 16 / (int64_t)x.element_size();
  auto stream = at::cuda::getCurrentCUDAStream();
  if (ml + mr == 0) {
    // full-width rows: one contiguous range per plane
    const int64_t start = mt * W, total = Hr * W;
    const auto cg = stats_grid(C, HW, total, slot_slack(vec, HW, start));
    const int64_t chunk = cg.first, gy = cg.second;
    AT_DISPATCH_FLOATING_TYPES_AND2(
        at::ScalarType::Half, at::ScalarType::BFloat16, x.scalar_type(),
        "bn_stats64_span", [&] {
          const dim3 grid((uint32_t)C, (uint32_t)gy);
          if (total == HW && planes_whole(vec, HW))
            hipLaunchKernelGGL((bn_stats64_kernel<scalar_t>), grid, dim3(256),
                               0, stream.stream(), x.data_ptr<scalar_t>(),
                               out.data_ptr<double>(), N, C, HW, chunk);
          else
            hipLaunchKernelGGL((bn_stats64_span_kernel<scalar_t>), grid,
                               dim3(256), 0, stream.stream(),
                               x.data_ptr<scalar_t>(), out.data_ptr<double>(),
                               N, C, HW, start, total, chunk);
        });
    return out;
  }
  TORCH_CHECK(HW < (int64_t)1 << 30, "plane too large");
  const int64_t len = W - ml - mr;
  const int64_t gy0 = stats_grid(C, HW, HW, 0).second;
  const int64_t rpc = (Hr + gy0 - 1) / gy0;
  const int64_t gy = (Hr + rpc - 1) / rpc;
  const int64_t S = len / vec + 2;  // slots a row can touch, at most
  // fast_div's exactness bound for both of the kernel's divisions
  TORCH_CHECK(N * rpc * S * std::max(S, rpc) < ((int64_t)1 << 32),
              "bn_stats64_region_acc: batch x rows x width too large");
  const uint32_t mS = (uint32_t)((((uint64_t)1) << 32) / (uint64_t)S + 1);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, x.scalar_type(),
      "bn_stats64_region_acc", [&] {
        hipLaunchKernelGGL((bn_stats64_region_kernel<scalar_t>),
                           dim3((uint32_t)C, (uint32_t)gy), dim3(256), 0,
                           stream.stream(), x.data_ptr<scalar_t>(),
                           out.data_ptr<double>(), N, C, HW, mt * W + ml,
                           (int)len, (int)W, (int)Hr, (int)rpc, (uint32_t)S,
                           mS);
      });
  return out;
}

torch::Tensor bn_stats64_acc(torch::Tensor x, torch::Tensor out) {
  return bn_stats64_region_acc(x, out, {0, 0, 0, 0});
}

torch::Tensor bn_stats64(torch::Tensor x) {
  check_bn_x(x);
  return bn_stats64_acc(
      x, torch::zeros({2 * x.size(1)}, x.options().dtype(torch::kDouble)));
}

torch::Tensor bn_apply(torch::Tensor x, torch::Tensor mean,
                       torch::Tensor invstd, torch::Tensor w, torch::Tensor b,
                       bool relu) {
  check_bn_x(x);
  const int64_t C = x.size(1), HW = x.size(2) * x.size(3);
  const int64_t total = x.numel();
  check_bn_vec(mean, C, "mean");
  check_bn_vec(invstd, C, "invstd");
  check_bn_vec(w, C, "w");
  check_bn_vec(b, C, "b");
  x = slot_aligned(x);
  auto y = torch::empty_like(x);
  const int64_t vec = 16 / (int64_t)x.element_size();
  auto stream = at::cuda::getCurrentCUDAStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, x.scalar_type(),
      "bn_apply", [&] {
        with_bool(relu, [&](auto relu_c) {
          with_bool(planes_whole(vec, HW), [&](auto whole_c) {
            hipLaunchKernelGGL(
                (bn_apply_kernel<scalar_t, decltype(relu_c)::value,
                                 decltype(whole_c)::value>),
                dim3(grid_for((total + vec - 1) / vec, 256)), dim3(256), 0,
                stream.stream(), x.data_ptr<scalar_t>(),
                y.data_ptr<scalar_t>(), mean.data_ptr<float>(),
                invstd.data_ptr<float>(), w.data_ptr<float>(),
                b.data_ptr<float>(), total, C, HW);
          });
        });
      });
  return y;
}

torch::Tensor bn_bwd_stats(torch::Tensor go, torch::Tensor x, torch::Tensor y,
                           torch::Tensor mean, torch::Tensor invstd,
                           bool relu,
                           c10::optional<torch::Tensor> zeroed = c10::nullopt) {
  check_bn_x(x);
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  check_bn_like(go, x, "go");
  if (relu) check_bn_like(y, x, "y");
  check_bn_vec(mean, C, "mean");
  check_bn_vec(invstd, C, "invstd");
  go = slot_aligned(go);
  x = slot_aligned(x);
  if (relu) y = slot_aligned(y);
  // `zeroed`: a caller-owned fp64 [2C] accumulator that holds zeros (the
  // one bn_finalize zero-filled for this forward); else a fresh fill
  torch::Tensor out;
  if (zeroed.has_value()) {
    out = *zeroed;
    check_bn_out(out, C);
    TORCH_CHECK(out.get_device() == x.get_device(),
                "bn: out must be on x's device");
  } else {
    out = torch::zeros({2 * C}, x.options().dtype(torch::kDouble));
  }
  const int64_t vec = 16 / (int64_t)x.element_size();
  const auto cg = stats_grid(C, HW, HW, slot_slack(vec, HW, 0));
  const int64_t chunk = cg.first, gy = cg.second;
  auto stream = at::cuda::getCurrentCUDAStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, x.scalar_type(),
      "bn_bwd_stats", [&] {
        with_bool(relu, [&](auto relu_c) {
          with_bool(planes_whole(vec, HW), [&](auto whole_c) {
            hipLaunchKernelGGL(
                (bn_bwd_stats_kernel<scalar_t, decltype(relu_c)::value,
                                     decltype(whole_c)::value>),
                dim3((uint32_t)C, (uint32_t)gy), dim3(256), 0, stream.stream(),
                go.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),
                relu ? y.data_ptr<scalar_t>() : (scalar_t*)nullptr,
                mean.data_ptr<float>(), invstd.data_ptr<float>(),
                out.data_ptr<double>(), N, C, HW, chunk);
          });
        });
      });
  return out;
}

// the launcher beneath bn_bwd_apply and bn_bwd_apply_region; `region`
// restricts the two reduction terms to rows [row_lo,row_hi) x cols
// [col_lo,col_hi)
//
// gsum / gxsum: the statistics as bn_bwd_stats made them (fp64, e.g. the
// two halves of its result) or their fp32 cast; both give the same bits.
// `pg` says where the launch puts the parameter gradients (none by default).
struct BnParamGrads {
  c10::optional<torch::Tensor> local;  // fp64 [2C]: this tile's own stats
  c10::optional<torch::Tensor> gw, gb; // fp32 [C] each: added into in place
  c10::optional<torch::Tensor> pgrad;  // fp32 [2C]: written where no gw/gb
};

static torch::Tensor bn_stat_f64(const torch::Tensor& v, int64_t C,
                                 const char* name) {
  TORCH_CHECK(v.is_cuda() && v.is_contiguous() && v.numel() == C &&
                  (v.scalar_type() == torch::kFloat ||
                   v.scalar_type() == torch::kDouble),
              "bn: ", name, " must be a contiguous fp32 or fp64 CUDA vector "
              "of ", C, " channels");
  return v.scalar_type() == torch::kDouble ? v : v.to(torch::kDouble);
}

static torch::Tensor bn_bwd_apply_launch(torch::Tensor go, torch::Tensor x,
                                         torch::Tensor y, torch::Tensor mean,
                                         torch::Tensor invstd, torch::Tensor w,
                                         torch::Tensor gsum,
                                         torch::Tensor gxsum, double n,
                                         bool relu, bool region, int row_lo,
                                         int row_hi, int col_lo, int col_hi,
                                         const BnParamGrads& pg) {
  check_bn_x(x);
  const int64_t C = x.size(1), W = x.size(3), HW = x.size(2) * W;
  const int64_t total = x.numel();
  check_bn_like(go, x, "go");
  if (relu) check_bn_like(y, x, "y");
  check_bn_vec(mean, C, "mean");
  check_bn_vec(invstd, C, "invstd");
  check_bn_vec(w, C, "w");
  gsum = bn_stat_f64(gsum, C, "gsum");
  gxsum = bn_stat_f64(gxsum, C, "gxsum");
  const double* local = nullptr;
  float *gw_acc = nullptr, *gb_acc = nullptr, *pgrad = nullptr;
  auto here = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.get_device() == x.get_device() &&
           t.is_contiguous();
  };
  if (pg.local.has_value()) {
    check_bn_out(*pg.local, C);
    TORCH_CHECK(here(*pg.local), "bn: local must be on x's device");
    local = pg.local->data_ptr<double>();
    auto sink = [&](const c10::optional<torch::Tensor>& t, const char* name) {
      if (!t.has_value()) return (float*)nullptr;
      TORCH_CHECK(here(*t) && t->scalar_type() == torch::kFloat &&
                      t->numel() == C,
                  "bn: ", name, " must be a contiguous fp32 vector of ", C,
                  " channels on x's device");
      return t->data_ptr<float>();
    };
    gw_acc = sink(pg.gw, "gw");
    gb_acc = sink(pg.gb, "gb");
    if (gw_acc == nullptr || gb_acc == nullptr) {
      TORCH_CHECK(pg.pgrad.has_value() && here(*pg.pgrad) &&
                      pg.pgrad->scalar_type() == torch::kFloat &&
                      pg.pgrad->numel() == 2 * C,
                  "bn: pgrad must be a contiguous fp32 vector of 2*C on x's "
                  "device when gw or gb is not given");
      pgrad = pg.pgrad->data_ptr<float>();
    }
  } else {
    TORCH_CHECK(!pg.gw.has_value() && !pg.gb.has_value() &&
                    !pg.pgrad.has_value(),
                "bn: gw, gb and pgrad need local");
  }
  go = slot_aligned(go);
  x = slot_aligned(x);
  if (relu) y = slot_aligned(y);
  auto gi = torch::empty_like(x);
  const int64_t vec = 16 / (int64_t)x.element_size();
  auto stream = at::cuda::getCurrentCUDAStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, x.scalar_type(),
      "bn_bwd_apply", [&] {
        with_bool(relu, [&](auto relu_c) {
          with_bool(region, [&](auto region_c) {
            with_bool(planes_whole(vec, HW), [&](auto whole_c) {
              hipLaunchKernelGGL(
                  (bn_bwd_apply_kernel<scalar_t, decltype(relu_c)::value,
                                       decltype(region_c)::value,
                                       decltype(whole_c)::value>),
                  dim3(grid_for((total + vec - 1) / vec, 256)), dim3(256), 0,
                  stream.stream(), go.data_ptr<scalar_t>(),
                  x.data_ptr<scalar_t>(),
                  relu ? y.data_ptr<scalar_t>() : (scalar_t*)nullptr,
                  gi.data_ptr<scalar_t>(), mean.data_ptr<float>(),
                  invstd.data_ptr<float>(), w.data_ptr<float>(),
                  gsum.data_ptr<double>(), gxsum.data_ptr<double>(), local,
                  gw_acc, gb_acc, pgrad, 1.0 / n, total, C, HW, (int)W, row_lo,
                  row_hi, col_lo, col_hi);
            });
          });
        });
      });
  return gi;
}

torch::Tensor bn_bwd_apply(torch::Tensor go, torch::Tensor x, torch::Tensor y,
                           torch::Tensor mean, torch::Tensor invstd,
                           torch::Tensor w, torch::Tensor gsum,
                           torch::Tensor gxsum, double n, bool relu,
                           c10::optional<torch::Tensor> local,
                           c10::optional<torch::Tensor> gw,
                           c10::optional<torch::Tensor> gb,
                           c10::optional<torch::Tensor> pgrad) {
  return bn_bwd_apply_launch(go, x, y, mean, invstd, w, gsum, gxsum, n, relu,
                             false, 0, 0, 0, 0, {local, gw, gb, pgrad});
}

// bn_bwd_apply when mean/var were taken over the region only
// (margin = top, bottom, left, right); n counts region pixels.
torch::Tensor bn_bwd_apply_region(torch::Tensor go, torch::Tensor x,
                                  torch::Tensor y, torch::Tensor mean,
                                  torch::Tensor invstd, torch::Tensor w,
                                  torch::Tensor gsum, torch::Tensor gxsum,
                                  double n, bool relu,
                                  std::vector<int64_t> margin,
                                  c10::optional<torch::Tensor> local,
                                  c10::optional<torch::Tensor> gw,
                                  c10::optional<torch::Tensor> gb,
                                  c10::optional<torch::Tensor> pgrad) {
  check_bn_x(x);
  const int64_t H = x.size(2), W = x.size(3);
  check_margin(margin, H, W);
  const bool region = margin[0] + margin[1] + margin[2] + margin[3] != 0;
  return bn_bwd_apply_launch(go, x, y, mean, invstd, w, gsum, gxsum, n, relu,
                             region, (int)margin[0], (int)(H - margin[1]),
                             (int)margin[2], (int)(W - margin[3]),
                             {local, gw, gb, pgrad});
}

// ---------------- state fan binding ----------------

// f(std::integral_constant<int, n>) for a run-time 0 <= n <= FAN_MAX
template <int I = 0, typename F>
static void with_count(int64_t n, F&& f) {
  if constexpr (I > FAN_MAX) {
    TORCH_CHECK(false, "fan_bwd: at most ", FAN_MAX, " terms of a kind");
  } else {
    if (n == I) f(std::integral_constant<int, I>{});
    else with_count<I + 1>(n, f);
  }
}

// g of fan_bwd_kernel. raw / rel: the gradients in fold order, each dense
// or a channel slice (go_plane_dense); r = relu(y), dense, needed when rel
// is not empty; slot = the number of raw terms folded before the masked sum.
torch::Tensor fan_bwd(std::vector<torch::Tensor> raw,
                      std::vector<torch::Tensor> rel,
                      c10::optional<torch::Tensor> r, int64_t slot) {
  const int64_t nraw = (int64_t)raw.size(), nrel = (int64_t)rel.size();
  TORCH_CHECK(nraw + nrel >= 1, "fan_bwd: no terms");
  TORCH_CHECK(nraw <= FAN_MAX && nrel <= FAN_MAX, "fan_bwd: at most ",
              FAN_MAX, " raw and ", FAN_MAX, " ReLU terms");
  TORCH_CHECK(slot >= 0 && slot <= nraw, "fan_bwd: slot outside the raw fold");
  const torch::Tensor& first = nraw ? raw[0] : rel[0];
  TORCH_CHECK(first.dim() == 4, "fan_bwd: terms are 4-D");
  const int64_t N = first.size(0), C = first.size(1);
  const int64_t HW = first.size(2) * first.size(3);
  const int64_t per_img = C * HW;
  const int64_t vec = 16 / (int64_t)first.element_size();
  bool vec_ok = HW % vec == 0;
  FanTerms t = {};
  auto take = [&](const torch::Tensor& a, const void*& p, int64_t& bs) {
    TORCH_CHECK(a.is_cuda() && a.sizes() == first.sizes() &&
                    a.scalar_type() == first.scalar_type() &&
                    a.get_device() == first.get_device() && go_plane_dense(a),
                "fan_bwd: every term is a CUDA tensor of one shape and dtype, "
                "dense or a channel slice of a contiguous tensor");
    p = a.data_ptr();
    bs = a.stride(0);
    vec_ok = vec_ok && aligned16(p) && bs % vec == 0;
  };
  for (int64_t k = 0; k < nraw; ++k) take(raw[k], t.raw[k], t.raw_bs[k]);
  for (int64_t k = 0; k < nrel; ++k) take(rel[k], t.rel[k], t.rel_bs[k]);
  const void* rp = nullptr;
  if (nrel) {
    TORCH_CHECK(r.has_value() && r->is_cuda() && r->is_contiguous() &&
                    r->sizes() == first.sizes() &&
                    r->scalar_type() == first.scalar_type() &&
                    r->get_device() == first.get_device(),
                "fan_bwd: r must be contiguous with the terms' shape and dtype");
    rp = r->data_ptr();
    vec_ok = vec_ok && aligned16(rp);
  }
  auto g = torch::empty(first.sizes(), first.options());
  if (g.numel() == 0) return g;
  TORCH_CHECK(N <= 65535, "fan_bwd: batch too large for the grid");
  vec_ok = vec_ok && aligned16(g.data_ptr());
  auto stream = at::cuda::getCurrentCUDAStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, first.scalar_type(),
      "fan_bwd", [&] {
        with_count(nraw, [&](auto nraw_c) {
          with_count(nrel, [&](auto nrel_c) {
            with_bool(vec_ok, [&](auto vec_c) {
              constexpr int V =
                  decltype(vec_c)::value ? 16 / (int)sizeof(scalar_t) : 1;
              hipLaunchKernelGGL(
                  (fan_bwd_kernel<scalar_t, decltype(nraw_c)::value,
                                  decltype(nrel_c)::value, V>),
                  dim3(grid_for(per_img / V, 256), (uint32_t)N), dim3(256), 0,
                  stream.stream(), t, (const scalar_t*)rp,
                  g.data_ptr<scalar_t>(), per_img, (int)slot);
            });
          });
        });
      });
  return g;
}

}  // namespace

void register_conv_mfma(pybind11::module_& m);
void register_conv_pw(pybind11::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_conv_mfma(m);
  register_conv_pw(m);
  m.def("halo_pack", &halo_copy<0>, "pack halo strips tile->flat buffer");
  m.def("halo_unpack", &halo_copy<1>, "unpack halo strips buffer->tile");
  m.def("halo_unpack_add", &halo_copy<2>, "accumulate grad strips into tile");
  m.def("bn_stats", &bn_stats, "per-channel [sum, sumsq] in one pass");
  namespace py = pybind11;
  m.def("maxpool_fwd", &maxpool_fwd, py::arg("x"), py::arg("k"), py::arg("s"),
        py::arg("p"), py::arg("force_generic") = false);
  m.def("maxpool_bwd", &maxpool_bwd, py::arg("go"), py::arg("idx"),
        py::arg("H"), py::arg("W"), py::arg("k"), py::arg("s"), py::arg("p"),
        py::arg("force_generic") = false);
  m.def("avgpool_fwd", &avgpool_fwd, py::arg("x"), py::arg("k"), py::arg("s"),
        py::arg("p"), py::arg("gr0"), py::arg("gc0"), py::arg("Hg"),
        py::arg("Wg"), py::arg("include_pad"),
        py::arg("force_generic") = false);
  m.def("avgpool_bwd", &avgpool_bwd, py::arg("go"), py::arg("H"), py::arg("W"),
        py::arg("k"), py::arg("s"), py::arg("p"), py::arg("gr0"),
        py::arg("gc0"), py::arg("Hg"), py::arg("Wg"), py::arg("include_pad"),
        py::arg("force_generic") = false);
  m.def("pool_kernel_name", &pool_kernel_name, py::arg("op"),
        py::arg("itemsize"), py::arg("H"), py::arg("W"), py::arg("k"),
        py::arg("s"), py::arg("p"), py::arg("aligned") = true,
        py::arg("go_bs") = 0,
        "label of the kernel the pool binding `op` (max_fwd, max_bwd, "
        "avg_fwd, avg_bwd) launches; plain integers, no HIP call");
  m.def("bn_stats64", &bn_stats64);
  m.def("bn_apply", &bn_apply);
  m.def("bn_bwd_stats", &bn_bwd_stats, py::arg("go"), py::arg("x"),
        py::arg("y"), py::arg("mean"), py::arg("invstd"), py::arg("relu"),
        py::arg("out") = py::none(),
        "fp64 [gsum, gxsum]; accumulated into `out` (zeroed, fp64 [2C]) when "
        "given, so no fill is launched");
  m.def("bn_bwd_apply", &bn_bwd_apply, py::arg("go"), py::arg("x"),
        py::arg("y"), py::arg("mean"), py::arg("invstd"), py::arg("w"),
        py::arg("gsum"), py::arg("gxsum"), py::arg("n"), py::arg("relu"),
        py::arg("local") = py::none(), py::arg("gw") = py::none(),
        py::arg("gb") = py::none(), py::arg("pgrad") = py::none(),
        "gi; with `local` (fp64 [2C]) the launch also adds the parameter "
        "gradients into gw / gb, or writes them to pgrad (fp32 [2C])");
  m.def("sgd_momentum", &sgd_momentum);
  m.def("bn_finalize", &bn_finalize, pybind11::arg("stats"),
        pybind11::arg("rmean"), pybind11::arg("rvar"),
        pybind11::arg("tracked"), pybind11::arg("mom"), pybind11::arg("n"),
        pybind11::arg("eps"), pybind11::arg("rezero") = false,
        pybind11::arg("zero2") = pybind11::none());
  m.def("bn_stats64_acc", &bn_stats64_acc);
  m.def("bn_stats64_region_acc", &bn_stats64_region_acc, py::arg("x"),
        py::arg("out"), py::arg("margin"));
  m.def("bn_bwd_apply_region", &bn_bwd_apply_region, py::arg("go"),
        py::arg("x"), py::arg("y"), py::arg("mean"), py::arg("invstd"),
        py::arg("w"), py::arg("gsum"), py::arg("gxsum"), py::arg("n"),
        py::arg("relu"), py::arg("margin"), py::arg("local") = py::none(),
        py::arg("gw") = py::none(), py::arg("gb") = py::none(),
        py::arg("pgrad") = py::none());
  m.def("fan_bwd", &fan_bwd, py::arg("raw"), py::arg("rel"), py::arg("r"),
        py::arg("slot"),
        "gradient of a fanned-out state: ordered fold of raw and ReLU-masked "
        "consumer gradients (ops/fuse.py)");
  m.attr("FAN_MAX") = (int)FAN_MAX;
  m.attr("gfx_arch") = "gfx950";
}
