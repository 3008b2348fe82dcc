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
//
// Split channels: tap_fwd_split_kernel<R, S, MF, ALIGNED> and
// tap_split_reduce_kernel, for grids that under-fill the device (a 64 x 64
// plane at N = 2 is 128 - 160 blocks of the kernel above). Opt-in:
// tap_fwd(split != 0).
//
// * The same body (tap_fwd_body: staging, tap addressing and fragment reads
//   are one piece of code), on a grid SC times as large: the slice index is
//   folded into the block index after the k tile. Slice sc runs the chunks
//   [first(sc), first(sc + 1)) of the ceil(C/32), dealt evenly with the
//   remainder to the earlier slices; SC <= chunks, so none is empty. Double
//   buffering and the one-tap-ahead weight loads are per slice.
// * Epilogue: the fp32 accumulators as they are, no bias, no rounding, to the
//   workspace part[SC][N][K][OH][OW] (a torch allocation of the launch),
//   through an fp32 [k][pixel] LDS image over the patch buffers, as many row
//   fragments a pass as fit them (3 for 1x7, 4 otherwise), then 16-byte row
//   stores where OW % 4 == 0, guarded element stores otherwise.
// * tap_split_reduce_kernel: out = bf16(part[0] + ... + part[SC-1] + bias),
//   added in that order in fp32: no atomics, bit-identical from run to run.
//   A thread takes 8 elements with 16-byte loads and one 16-byte store where
//   OH*OW % 8 == 0, one element otherwise.
// * Chooser (tap_split_choice, the one place). With the unsplit kernel's MF,
//   a grid of at least 2 blocks per CU stays unsplit: SC = 1. Otherwise MF is
//   the unsplit chooser's but 4 in place of 7 (about 148 + 64 registers: two
//   waves per SIMD, and 7 k tiles where MF = 7 has 4), and SC is the smallest
//   of 1 .. min(chunks, 8) that reaches 2 blocks per CU, or the largest
//   allowed if none does. If that SC is 1 the launch is the unsplit kernel
//   with its own MF. A forced slice count uses the same MF.
//
// Strided: tap_strided_fwd_kernel<R, S, MF, ALIGNED> and
// tap_strided_bwd_data_kernel<R, S, MF, ALIGNED>, for 1x7 at stride (1, 2),
// 7x1 at (2, 1) and 3x3 at (2, 2) (sh = 2 where R > 1, sw = 2 where S > 1),
// the same pads, Wt and pre-pass. Opt-in: tap_fwd_strided,
// tap_bwd_data_strided.
//
// * Forward. The scheme above (32-channel chunks, double-buffered patch, k over
//   the channels of one tap, weights one tap ahead in registers, bf16 epilogue
//   over the patch) on a patch of ((TH-1)*sh + R) x ((TW-1)*sw + S) pixels. A
//   B fragment is 16 consecutive output columns: input columns sw apart. On
//   the [row][col] image that read steps 160 bytes a lane, 40 banks: lane i
//   starts on bank 40*i mod 64 = 0,40,16,56,32,8,48,24 and again 0: lanes i
//   and i + 8 share a 4-bank span, a 2-way conflict on every tap. So the patch
//   is staged phase-split: patch column lc lies in column plane lc % sw at
//   index lc / sw, patch row lr in row plane lr % sh at lr / sh, every plane
//   [row][col][32 ch] at 80 bytes a pixel. Output column j of tap s is patch
//   column j*sw + cc, cc = PADL - pw + s: plane cc % sw, index j + cc / sw,
//   the same plane for all 16 lanes and one pixel a lane. Tap (r, s) of
//   fragment (row, col0) is again one ds_read_b128, at
//   plane(r % sh, cc % sw) + ((row + r/sh) * PWP + col0 + (lane & 15) + cc/sw)
//   * 80 B + (lane >> 4) * 16 B: lane i starts on bank 20*i mod 64 =
//   0,20,40,60,16,36,56,12,32,52,8,28,48,4,24,44, sixteen disjoint 4-bank
//   spans at every constant offset, as at stride 1.
//   The de-interleave is free on the ALIGNED path: each of the eight
//   ds_write_b128 after the v_perm transpose carries one pixel, and pixel p of
//   a group goes to plane p % sw, p / sw pixels on. The patch has more than
//   256 (row, 8 pixels, 8 channels) items: two a thread. By elements wave cg
//   stages channel group cg, a lane one pixel per ds_write_b128.
// * Tiles and LDS (80 B a pixel, two buffers; PWL = columns in LDS):
//     1x7  4 x 64   patch  4 x 133, PWL 144: 2 planes of  4 x 72   92160 B
//     7x1  8 x 32   patch 21 x  32, PWL  32: 2 planes of 11 x 32  112640 B
//     3x3  4 x 32   patch  9 x  65, PWL  80: 4 planes of  5 x 40  128000 B
//   3x3 at the stride-1 tile, 8 x 32, is 17 x 80 pixels, 2 x 108800 B, over
//   the 160 KB; 8 x 16 is 17 x 48, 130560 B and 6.4 staged pixels per output
//   pixel where 4 x 32 has 5.6. So 3x3 runs 8 fragments a tile, two a wave,
//   and a weight fragment feeds 2 MFMAs, not 4. MF is the stride-1 chooser's.
// * Data gradient, by phase decomposition:
//     gx[h][w] = sum_k sum_(r,s) go[k][(h+ph-r)/sh][(w+pw-s)/sw] * w[k][c][r][s]
//   over the taps with r = (h + ph) mod sh and s = (w + pw) mod sw. The taps
//   of class (ra, rb) = (r % sh, s % sw) serve exactly the gx pixels of phase
//   a = (ra - ph) mod sh, b = (rb - pw) mod sw: 4 + 3 taps for the 1-D
//   filters, 4 + 2 + 2 + 1 for 3x3, and each class is a stride-1 tap-shift
//   convolution of go. Tap r = ra + sh*m of the class reads go row
//   i + (a + ph - ra)/sh - m for the gx row i*sh + a.
//   All phases in one block (the baseline; none spilled, so the
//   phase-per-block grid, which restages go sh*sw times, was not built): a
//   block owns TH x TW phase cells (go pixels), TH*sh x TW*sw pixels of gx,
//   with the tiles of the forward. It stages the go patch once per 32-channel
//   chunk of K in the plain stride-1 layout, (TH + (R-1)/sh + sh-1) rows x
//   (TW + (S-1)/sw + sw-1) columns (4 x 68, 12 x 32, 6 x 34: at most 2 x
//   30720 B), and walks all R*S taps class by class against it, each class
//   into its own accumulators: sh*sw * MF * NF fragments, so MF is at most 4
//   for 3x3 (128 registers; 1x7 and 7x1 at MF = 7: 224). Wt is the transposed
//   pre-pass as it is; a class only selects the tap indices.
//   Epilogue: the classes interleaved in the [c][pixel] image of the gx tile
//   (116480 B at MF = 7, over the patch), pixel (row*sh + a, col*sw + b), then
//   16-byte row stores where W % 8 == 0, guarded element stores otherwise.
//   Every pixel of [0, H) x [0, W) is written: go outside its extents is
//   staged as zeros, which makes borders, and the rows and columns that no
//   filter position reaches, exact zeros. No atomics, fixed summation order.
//
// Weight gradient: tap_bwdw_kernel<R, S, XAL, GAL>
//
//   gw[k][c][r][s] += sum_{n,oh,ow} go[n][k][oh][ow] * x[n][c][oh-ph+r][ow-pw+s]
//
// The forward turned around: the MFMA's k is now 32 pixels of one tile row.
// For one tap it is the GEMM GO[k][pixels] * X_t[c][pixels]^T, and the R*S
// taps differ only by a whole-pixel shift of X, so go and the x patch are
// staged once per pixel tile and a tap is a constant added to the address of
// the x fragment.
//
// * Block (256 threads): 64 output channels x 64 input channels x all taps
//   of gw, and a contiguous run of `tpb` pixel tiles (over images, tile rows,
//   tile columns) of TH x TW = 2 x 64 (1x7) or 4 x 32 (7x1, 3x3) pixels: half
//   of Tile<R,S>, because both operands of a 256-pixel tile do not fit the
//   160 KB of LDS twice. Accumulators stay in registers over the run; the
//   block ends with fp32 atomicAdd into gw.
// * Waves split the block by input channels: wave w owns x channels
//   c0 + 16w .. +16, all 64 go channels and all taps, 4 x R*S accumulator
//   fragments (112 / 144 registers). Per 32-pixel k-step a wave reads 4 go
//   fragments and R*S x fragments for 4 * R*S MFMAs: 0.79 (1x7, 7x1) / 0.72
//   (3x3) fragment reads per MFMA and no reduction between waves. The two
//   splits the design note names cost: by output rows 2.1 reads per MFMA; by
//   pixels (64 x 32 tile, 224 registers a lane) 0.64 but an LDS reduction of
//   3 x 57 KB, and it spilled in every instantiation (48 - 816 bytes a lane).
// * Fragments: ds_read_b64_tr_b16 with per-lane row addresses. Lane l of a
//   16-lane group points at pixel p0 + ((l&15)>>2), channels c + (l&3)*4 and
//   receives channel c + (l&15) at pixels p0 .. p0+3. Group g takes
//   p0 = 4g for the first read and 16 + 4g for the second, the same for go
//   and x, so the MFMA's k slot 8g + e is pixel 4g + e (e < 4) or
//   16 + 4g + e - 4: any order does, as long as A and B agree.
// * LDS pixel stride: 160 bytes for both images (64 channels + 32 bytes).
//   64 banks of 4 bytes; a 16-lane group touches 4 pixels x 32 bytes, and
//   with the group order above lanes 0 - 31 touch 8 consecutive pixels
//   p .. p+7 x 32 bytes = 256 bytes, one pass of all banks if the 8 spans are
//   disjoint. A stride of 32*m bytes puts pixel p on span (p*m) mod 8, so m
//   must be odd: m = 5 gives 0,5,2,7,4,1,6,3. (128 bytes, m = 4, would put
//   every second pixel on the same span; with the textbook group order, p0 =
//   8g, pixels p and p+8 collide for every m.) A tap adds the same offset to
//   all lanes, so it keeps this. Rows are 128 bytes longer than their pixels:
//   the 16 lanes of a staging ds_write_b128 pass are 8 channel groups x 2
//   rows, and whole rows are multiples of 256 bytes apart without it.
// * Staging: the forward's, as a second copy (struct Operand) used for both
//   images: the tile moves every step, so offsets and masks are per step, the
//   stride differs, and the pixel tail of go is one more mask. The forward
//   keeps its own copy, so its code is unchanged. go and x each choose the
//   16-byte path on their own (W % 8 resp. OW % 8, base alignment). Double
//   buffered: loads of tile i+1 before the MFMAs of tile i, commit after
//   them, one barrier per tile.
//   x by elements is staged in two passes a step (the second is loaded when
//   the first is committed, half way through the MFMAs): in one pass the 3x3
//   kernel spilled.
// * Only go is zeroed past OH / OW: the x values paired with those pixels are
//   real image values times zero. A non-finite x there gives NaN in taps whose
//   true sum does not touch it (conv2d_weight stays finite): inputs are
//   assumed finite, as in conv_bwd_weight.
// * Grid: tpb is chosen on the host so that the grid is about 2 blocks per CU
//   (256 CUs) and at least one per CU where the problem has that many
//   (output tile, pixel tile) pairs.
//
// Weight gradient, rolling window: tap_bwdw_ring_kernel<R, S, NARROW, XAL, GAL>
//
// The same GEMM, fragments, k-slot order and staging (struct Operand,
// unchanged) on a block small enough that two are resident on a CU, and that
// stages every x row once.
//
// * Block (256 threads): 32 output channels x 64 input channels (NARROW: 32 x
//   32) x all taps, and one strip: a band of TW = 64 (1x7) or 32 (7x1, 3x3)
//   output columns of one image over `rows` consecutive output rows, walked
//   downwards in steps of TH = 2 rows (128 / 64 pixels between barriers).
// * Waves: by input channels, 16 each, KF = 2 go fragments: 2 x R*S
//   accumulator fragments (56 / 72 registers), 2 + R*S fragment reads for
//   2 * R*S MFMAs per k-step. NARROW: 2 x 2 over go and x fragments, R*S
//   accumulators (28 / 36), 1 + R*S reads for R*S MFMAs.
// * Ring. Rows are staged in units of TH. Step i reads go unit i and x units
//   i .. i + D, D = ceil((R - 1) / TH) = 0 / 3 / 1, and while it computes,
//   unit i + 1 + D is committed: SLOTS = D + 2 units of x (4 / 10 / 6 rows)
//   and 2 of go. Unit u lies in slot u mod SLOTS, so a unit never wraps and
//   staging writes whole units; patch row q of step i is ring row
//   (i*TH mod RROWS) + q, minus RROWS where that is past the end: one
//   compare-and-subtract on a uniform value per patch row and step, then the
//   tap is the old constant offset. For 1x7, D = 0: plain double buffering.
// * Prefetch. x on the 16-byte path has two register sets: the loads of step
//   i + 2 are issued at the top of step i and committed at the end of step
//   i + 1, into the slot last read in step i - 1. go, and x by elements, are
//   loaded at the top of step i and committed at its end (one step ahead, one
//   set): with two sets of each the wide instantiations spilled. One barrier
//   per step.
// * LDS: go 96 bytes a pixel (32 channels + 32 bytes: 32*3, odd, so the same
//   span argument as above holds: 0,3,6,1,4,7,2,5), x 160 (NARROW: 96); rows
//   128 bytes longer. go 2 units + x SLOTS units:
//     1x7  4 * 6272 + 4 * 12928 = 76800 B   (NARROW 56320)
//     7x1  4 * 3200 + 10 * 5248 = 65280 B   (NARROW 44800)
//     3x3  4 * 3200 + 6 * 7808  = 59648 B   (NARROW 41216)
//   all at most 80 KB, and __launch_bounds__(256, 2) holds the registers to
//   256 a lane: two blocks per CU.
// * Grid: k and c tiles of a strip innermost (one XCD's L2), then strips,
//   bands, images. The strip length is chosen on the host so that the grid is
//   at least 4 x 256 blocks where the problem has that many steps.
// * NARROW is chosen where C rounded up to 32 is less than C rounded up to 64
//   (C = 20: 32 against 64; C = 52 is 64 under both and stays wide), and
//   wherever x is staged by elements (W % 8 != 0 or an unaligned base): the
//   three of the wide tile's six such instantiations spilled 96 - 352 bytes a
//   lane, and none of the six is built.
//
// Weight gradient, pixel-major: tap_bwdw_px_kernel<R, S, XAL, GAL>
//
// The same GEMM with both operands staged as they lie in NCHW memory,
// [channel][row][column]: the MFMA's k is 32 consecutive pixels of a row, and
// a lane's 8 k values are 16 contiguous bytes of one channel, so there is no
// transpose on the way into LDS (no v_perm) and none on the way out (plain
// ds_read_b128, no ds_read_b64_tr_b16).
//
// * Block (256 threads): 128 output channels x 32 input channels x all taps
//   and one strip, as in the ring kernel: a band of TW = 64 (1x7) or 32 (7x1,
//   3x3) output columns over `rows` output rows, walked downwards in steps of
//   TH = 2 (1x7) or 4 rows, 128 pixels between barriers. Where K <= 128, x is
//   staged once per pixel for all of K; go is staged once per 32 channels of x.
// * Waves: by go fragments, two each, with both x fragments and all taps:
//   4 x R*S accumulator fragments (112 / 144 registers), 2 go reads and 2 x
//   (R: 1 / 7 / 3) x (3 window reads, for 7x1 one) for 4 * R*S MFMAs a k-step.
//   A wave whose go channels all lie past K only stages.
// * Fragments: lane l reads channel (l & 15) at pixels p0 + 8 * (l >> 4) .. + 8.
//   A row tap is a row offset in the address. Column taps: the patch starts
//   PADL = 8 columns left of the band; per (x fragment, row, k-step) the lane
//   reads the three aligned 8-pixel groups around its own, 12 registers, and
//   tap s starts at element 8 + s - S/2 of them: an even start is four of the
//   registers as they are, an odd one four v_alignbit_b32 (1x7: 16 of them for
//   7 fragments, 3x3: 8 for 3). The starts are constants for the pad S/2; any
//   other pw stages x by elements with the image moved S/2 - pw columns under
//   the patch, so there is one compute loop per filter shape.
// * LDS: a channel is its pixels rounded up to an odd number of 16-byte groups
//   (go 272 bytes; x 336 / 656 / 592), so 16 consecutive channels at one pixel
//   offset start on 16 different 16-byte spans of the 256-byte bank row. Two
//   buffers of go (34816 B) and x: 91136 / 111616 / 107520 B, one block a CU.
// * Staging (struct PxOperand): an item is 8 pixels of one row of one channel,
//   one ds_write_b128. 16-byte path (W % 8 == 0, aligned base, for x also
//   pw == S/2; OW % 8 == 0 for go): one 16-byte load an item, issued before the
//   MFMAs of a step and masked and written after them, one barrier a step. By
//   elements: eight clamped 2-byte loads and a mask per pixel, staged after the
//   MFMAs without prefetch (held across them, 5 of the 8 such instantiations
//   spilled). Zeros: pads, borders, go past OW and below the strip, channel
//   tails. As above, x paired with zeroed go is real image data: finite inputs.
// * Grid: as the ring kernel's, with the strip length chosen for at least
//   2 x 256 blocks where the problem has that many steps.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <tuple>
#include <utility>

namespace conv_tap {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;

constexpr int CK = 32;    // channels per chunk (MFMA k)
constexpr int PSTR = 40;  // shorts per patch pixel: 32 channels + 8 of padding

struct TapGeom {
  int N, C, H, W;  // input (C is the reduction dim of this launch)
  int K;           // output channels of this launch
  int OH, OW, ph, pw;
  int Kp, Cp;      // padded extents of Wt
  int row_blocks, col_blocks, k_tiles;
  int vec_out;     // 16-byte row stores are possible
  int sc;          // channel slices (tap_fwd_split_kernel only)
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

// The body of tap_fwd_kernel and of tap_fwd_split_kernel. SPLIT: the block
// runs only its slice of the channel chunks and leaves its fp32 accumulators
// in `part` (bias and out are not used); otherwise all chunks, and bias,
// rounding and `out` as described above (`part` is not used).
template <int R, int S, int MF, bool ALIGNED, bool SPLIT>
__device__ __forceinline__ void tap_fwd_body(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ Wt,
    const float* __restrict__ bias, unsigned short* __restrict__ out,
    float* __restrict__ part, const TapGeom& g) {
  using T = Tile<R, S>;
  constexpr int TH = T::TH, TW = T::TW, PH = T::PH, PADL = T::PADL;
  constexpr int PWN = T::PWN, PWL = T::PWL, PBUF = T::PBUF, ES = T::ES;
  constexpr int RS = R * S;
  constexpr int KB = MF * 16;         // output channels per block
  constexpr int FPR = TW / 16;        // fragments per tile row
  constexpr int NF = TH * FPR / 4;    // fragments per wave
  static_assert(NF == 4, "16 fragments per tile, four per wave");
  // SPLIT: the fp32 epilogue image takes EP row fragments at a time, as many
  // as fit the patch buffers, so the split kernel needs no more LDS
  constexpr int ESF = TH * TW + 4;    // its row stride in floats
  constexpr int EPFIT = PBUF / (16 * ESF);
  constexpr int EP = MF < EPFIT ? MF : EPFIT;
  static_assert(EP >= 1, "one row fragment of the fp32 image fits");
  constexpr int LDS_SHORTS =
      SPLIT || 2 * PBUF > KB * ES ? 2 * PBUF : KB * ES;

  // block -> (k tile, [channel slice,] column block, row block, image),
  // XCD-aware bijective swizzle as in conv_fwd_kernel
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int xcd = blockIdx.x & 7, sub = blockIdx.x >> 3;
  int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + sub;
  if (bid >= nwg) bid = blockIdx.x;  // never taken: the mapping is bijective
  const int kt = bid % g.k_tiles;
  bid /= g.k_tiles;
  // this block's chunks [ch_b, ch_e): all of them, or slice sc of g.sc, dealt
  // evenly with the remainder to the earlier slices (g.sc <= chunks: >= 1)
  const int chunks = g.Cp / CK;
  int sc = 0, ch_b = 0, ch_e = chunks;
  if constexpr (SPLIT) {
    sc = bid % g.sc;
    bid /= g.sc;
    const int q = chunks / g.sc, rem = chunks % g.sc;
    ch_b = sc * q + (sc < rem ? sc : rem);
    ch_e = ch_b + q + (sc < rem ? 1 : 0);
  }
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
  stage_load(ch_b * CK);
  load_a(a_cur, 0, ch_b * CK);
  stage_commit(0, ch_b * CK);
  __syncthreads();

  for (int ch = ch_b; ch < ch_e; ++ch) {
    const int buf = (ch - ch_b) & 1;
    const bool more = ch + 1 < ch_e;
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

  // ---- epilogue of a slice: the accumulators as they are, to part[sc] -------
  // F image: [k][pixel] fp32 over the patch buffers, EP row fragments a pass,
  // rows ESF floats apart (4 rows are 16 banks apart: the four 16-lane groups
  // of a write do not collide). item = (k, 4-pixel segment).
  if constexpr (SPLIT) {
    float* F = (float*)lds;
    constexpr int SEG4 = TH * TW / 4;
    const int64_t OHW = (int64_t)g.OH * g.OW;
    float* pn = part + ((int64_t)sc * g.N + n) * g.K * OHW;
#pragma unroll
    for (int m0 = 0; m0 < MF; m0 += EP) {
      if (m0 > 0) __syncthreads();  // the reads of the pass before
#pragma unroll
      for (int e = 0; e < EP; ++e) {
        const int mf = m0 + e < MF ? m0 + e : MF - 1;
        if (m0 + e < MF) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int k = e * 16 + ((lane >> 4) << 2) + reg;
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
              const int f = wid * NF + nf;
              const int pix = (f / FPR) * TW + (f % FPR) * 16 + (lane & 15);
              F[k * ESF + pix] = acc[mf][nf][reg];
            }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < EP * 16 * SEG4 / 256; ++it) {
        const int idx = it * 256 + tid;
        const int seg = idx % SEG4, k = idx / SEG4;
        const int kout = k0 + m0 * 16 + k;
        const int oh = oh0 + seg / (TW / 4), ow = ow0 + (seg % (TW / 4)) * 4;
        if (m0 * 16 + k >= KB || kout >= g.K || oh >= g.OH || ow >= g.OW)
          continue;
        const f32x4 v = *(const f32x4*)(F + k * ESF + seg * 4);
        float* dst = pn + (int64_t)kout * OHW + (int64_t)oh * g.OW + ow;
        if (g.vec_out) {  // OW % 4 == 0: the segment is whole
          *(f32x4*)dst = v;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (ow + e < g.OW) dst[e] = v[e];
        }
      }
    }
    return;
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

template <int R, int S, int MF, bool ALIGNED>
__global__ __launch_bounds__(256) void tap_fwd_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ Wt,
    const float* __restrict__ bias, unsigned short* __restrict__ out,
    TapGeom g) {
  tap_fwd_body<R, S, MF, ALIGNED, false>(x, Wt, bias, out, nullptr, g);
}

// ---------------------------------------------------------------------------
// Split channels (header: "Split channels")
// ---------------------------------------------------------------------------

// MF <= 4 and two blocks a CU: at most 76800 B of LDS, and the registers held
// to 256 a lane, except for MF = 4 by elements, which then spilled 18 - 77
// registers a lane
template <int R, int S, int MF, bool ALIGNED>
__global__ __launch_bounds__(256, (ALIGNED || MF < 4) ? 2 : 1)
void tap_fwd_split_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ Wt,
    float* __restrict__ part, TapGeom g) {
  tap_fwd_body<R, S, MF, ALIGNED, true>(x, Wt, nullptr, nullptr, part, g);
}

// out[i] = bf16(part[0][i] + part[1][i] + ... + part[sc-1][i] + bias[k(i)]),
// summed in that order in fp32, i over the `total` = N*K*OH*OW elements.
// VEC (OH*OW % 8 == 0, 16-byte aligned bases): a thread takes 8 elements of
// one (image, channel) plane, two 16-byte loads a slice and one 16-byte store;
// otherwise one element a thread.
template <bool VEC>
__global__ __launch_bounds__(256) void tap_split_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ bias,
    unsigned short* __restrict__ out, int sc, int K, int64_t OHW,
    int64_t total) {
  constexpr int E = VEC ? 8 : 1;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * E;
  if (i >= total) return;
  const float b = bias ? bias[(i / OHW) % K] : 0.f;
  if constexpr (VEC) {
    f32x4 lo = *(const f32x4*)(part + i), hi = *(const f32x4*)(part + i + 4);
    for (int s = 1; s < sc; ++s) {
      const float* p = part + s * total + i;
      const f32x4 l = *(const f32x4*)p, h = *(const f32x4*)(p + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lo[e] += l[e];
        hi[e] += h[e];
      }
    }
    i32x4 o;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      o[j] = pack_bf16(lo[2 * j] + b, lo[2 * j + 1] + b);
      o[j + 2] = pack_bf16(hi[2 * j] + b, hi[2 * j + 1] + b);
    }
    *(i32x4*)(out + i) = o;
  } else {
    float v = part[i];
    for (int s = 1; s < sc; ++s) v += part[s * total + i];
    out[i] = (unsigned short)(pack_bf16(v + b, 0.f) & 0xffff);
  }
}

// ---------------------------------------------------------------------------
// Weight gradient (header: "Weight gradient: tap_bwdw_kernel")
// ---------------------------------------------------------------------------

struct WgGeom {
  int N, C, H, W, K, OH, OW, ph, pw;
  int row_blocks, col_blocks;  // pixel tiles of one image
  int tiles;                   // N * row_blocks * col_blocks
  int tpb;                     // tiles per block (the run length)
  int k_tiles, c_tiles;
};

template <int R, int S>
struct WgTile {
  using T = Tile<R, S>;
  static constexpr int KF = 4, CF = 4;  // 16-channel fragments of go and of x
  static constexpr int TH = T::TH / 2;  // half the forward's tile: LDS
  static constexpr int TW = T::TW;
  static constexpr int PH = TH + R - 1;
  static constexpr int STR = 80;                     // shorts per pixel
  static constexpr int GROW = TW * STR + 64;         // shorts per go row
  static constexpr int XROW = T::PWL * STR + 64;     // shorts per patch row
  static constexpr int GBUF = TH * GROW;
  static constexpr int BUF = GBUF + PH * XROW;       // one step: go, then x
  static constexpr int LDS_SHORTS = 2 * BUF;
  static_assert(TW % 32 == 0, "a k-step is 32 pixels of one tile row");
  static_assert(LDS_SHORTS * 2 <= 160 * 1024, "LDS of one CU");
};

// One operand of a step: ROWS x COLS pixels x NG*8 channels of an NCHW image,
// staged as [row][column][channel], STR shorts per pixel and ROW per row. The
// second copy of tap_fwd_kernel's staging (same loads, same v_perm transpose,
// same masks at commit); what differs is that the tile moves every step, so
// only `soff` is kept between load and commit and the rest is recomputed.
// ALIGNED: an item is (8-channel group, row, 8-pixel group of the COLS_L
// columns in LDS). Otherwise (column of the COLS_N needed ones, 8-channel
// group, row). The items of a thread are loaded and committed in NP passes, so
// that only PP of them are in registers at a time.
template <int ROWS, int COLS_L, int COLS_N, int NG, int STR, int ROW,
          bool ALIGNED, int NP = 1>
struct Operand {
  static constexpr int ITEMS =
      ALIGNED ? ROWS * (COLS_L / 8) * NG : ROWS * COLS_N * NG;
  static constexpr int PT = (ITEMS + 255) / 256;  // items per thread
  static constexpr int PP = (PT + NP - 1) / NP;   // items per pass
  int soff[PT];  // offset in the channel plane; -1: outside the image
  i32x4 rawv[ALIGNED ? PP : 1][8];
  unsigned raws[ALIGNED ? 1 : PP][8];

  static __device__ __forceinline__ void split(int u, int& row, int& col,
                                               int& cg) {
    if constexpr (ALIGNED) {
      cg = u % NG;
      row = (u / NG) % ROWS;
      col = (u / NG) / ROWS * 8;
    } else {
      col = u % COLS_N;
      cg = (u / COLS_N) % NG;
      row = (u / COLS_N) / NG;
    }
  }

  // (row0, col0): image coordinates of row 0 and of column index 0
  __device__ __forceinline__ void locate(int tid, int row0, int col0, int Hi,
                                         int Wi) {
#pragma unroll
    for (int it = 0; it < PT; ++it) {
      int row, col, cg;
      split(it * 256 + tid, row, col, cg);
      const int ih = row0 + row, iw = col0 + col;
      // ALIGNED: Wi % 8 == 0 and iw % 8 == 0, a group is wholly in or out
      const bool ok = it * 256 + tid < ITEMS && ih >= 0 && ih < Hi && iw >= 0 &&
                      iw < Wi;
      soff[it] = ok ? ih * Wi + iw : -1;
    }
  }

  // issue the loads of channels c0 .. c0 + NG*8 (clamped below Cmax: always
  // inside the image); nothing is read of them before `commit`
  // (32-bit offsets from a uniform base: an image has fewer than 2^31 elements)
  template <int PASS = 0>
  __device__ __forceinline__ void load(const unsigned short* img, int HW,
                                       int c0, int Cmax, int tid) {
    constexpr int B = PASS * PP;
#pragma unroll
    for (int it = B; it < PT && it < B + PP; ++it) {
      if (it * 256 + tid >= ITEMS) continue;
      int row, col, cg;
      split(it * 256 + tid, row, col, cg);
      const int off = soff[it] < 0 ? 0 : soff[it];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + cg * 8 + e;
        const unsigned short* p =
            img + (unsigned)((c < Cmax ? c : Cmax - 1) * HW + off);
        if constexpr (ALIGNED)
          rawv[it - B][e] = *(const i32x4*)p;
        else
          raws[it - B][e] = *p;
      }
    }
  }

  // lc0: LDS column of column index 0. Pads, borders, the pixel tail and the
  // channel tail become zeros here.
  template <int PASS = 0>
  __device__ __forceinline__ void commit(short* buf, int c0, int Cmax, int lc0,
                                         int tid) {
    constexpr int B = PASS * PP;
#pragma unroll
    for (int it = B; it < PT && it < B + PP; ++it) {
      if (it * 256 + tid >= ITEMS) continue;
      int row, col, cg;
      split(it * 256 + tid, row, col, cg);
      const unsigned sm = soff[it] < 0 ? 0u : ~0u;
      unsigned cm[4];  // dword j holds channels 2j (low) and 2j + 1
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + cg * 8 + 2 * j;
        cm[j] = sm & ((c < Cmax ? 0xffffu : 0u) | (c + 1 < Cmax ? 0xffff0000u : 0u));
      }
      short* dst = buf + row * ROW + (lc0 + col) * STR + cg * 8;
      if constexpr (ALIGNED) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          // 8x8 transpose of 16-bit values: pixel p of channels 2j and 2j+1
          const unsigned sel = (p & 1) ? 0x07060302u : 0x05040100u;
          i32x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            o[j] = (int)(__builtin_amdgcn_perm(
                             (unsigned)rawv[it - B][2 * j + 1][p >> 1],
                             (unsigned)rawv[it - B][2 * j][p >> 1], sel) &
                         cm[j]);
          *(i32x4*)(dst + p * STR) = o;
        }
      } else {
        i32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = (int)((raws[it - B][2 * j] | (raws[it - B][2 * j + 1] << 16)) &
                       cm[j]);
        *(i32x4*)dst = o;
      }
    }
  }
};

// MFMA operand fragment of 16 channels x 32 pixels from a channel-innermost
// image: p points at (pixel p0 + 4*(lane>>4) + ((lane&15)>>2), channel
// c0 + (lane&3)*4); the lane receives channel c0 + (lane&15) at pixels
// p0 + 4*(lane>>4) + {0..3} and, `half` shorts further, at those + 16.
__device__ __forceinline__ s16x8 read_tr16(const short* p, int half) {
  auto* q = (__attribute__((address_space(3))) short*)p;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)q);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(q + half));
  s16x8 frag;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    frag[e] = lo[e];
    frag[e + 4] = hi[e];
  }
  return frag;
}

template <int R, int S, bool XAL, bool GAL>
__global__ __launch_bounds__(256) void tap_bwdw_kernel(
    const unsigned short* __restrict__ go, const unsigned short* __restrict__ x,
    float* __restrict__ gw, WgGeom g) {
  using T = WgTile<R, S>;
  using FT = Tile<R, S>;
  constexpr int RS = R * S, KF = T::KF, CF = T::CF;
  constexpr int TH = T::TH, TW = T::TW, PADL = FT::PADL;
  constexpr int STR = T::STR, GROW = T::GROW, XROW = T::XROW;
  constexpr int KPR = TW / 32;           // k-steps (32 pixels) per tile row
  constexpr int KS = TH * KPR;           // k-steps per tile
  static_assert(CF == 4, "one 16-channel fragment of x per wave");

  __shared__ __attribute__((aligned(16))) short lds[T::LDS_SHORTS];

  // block -> (k tile, c tile, run of pixel tiles); XCD-aware bijective swizzle
  // as in tap_fwd_kernel, so the blocks that share a run share an L2
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int xcd = blockIdx.x & 7, sub = blockIdx.x >> 3;
  int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + sub;
  if (bid >= nwg) bid = blockIdx.x;  // never taken: the mapping is bijective
  const int k0 = (bid % g.k_tiles) * (KF * 16);
  bid /= g.k_tiles;
  const int c0 = (bid % g.c_tiles) * (CF * 16);
  const int run = bid / g.c_tiles;
  const int t_begin = run * g.tpb;
  const int t_end = t_begin + g.tpb < g.tiles ? t_begin + g.tpb : g.tiles;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int HW = g.H * g.W, OHW = g.OH * g.OW;

  Operand<TH, TW, TW, KF * 2, STR, GROW, GAL> sg;
  // x by elements is 5 - 10 items a thread: staged in two passes, the second
  // loaded when the first is committed, half way through the MFMAs
  constexpr int NPX = XAL ? 1 : 2;
  Operand<T::PH, FT::PWL, FT::PWN, CF * 2, STR, XROW, XAL, NPX> sx;
  const unsigned short* xn = x;  // image of the tile being staged
  auto stage_load = [&](int tl) {
    const int cb = tl % g.col_blocks;
    tl /= g.col_blocks;
    const int rb = tl % g.row_blocks, n = tl / g.row_blocks;
    const int oh0 = rb * TH, ow0 = cb * TW;
    sg.locate(tid, oh0, ow0, g.OH, g.OW);
    sx.locate(tid, oh0 - g.ph, XAL ? ow0 - PADL : ow0 - g.pw, g.H, g.W);
    sg.load(go + (int64_t)n * g.K * OHW, OHW, k0, g.K, tid);
    xn = x + (int64_t)n * g.C * HW;
    sx.load(xn, HW, c0, g.C, tid);
  };
  // two passes: x's first into `buf`, then the loads of its second
  auto stage_middle = [&](int buf) {
    if constexpr (NPX == 2) {
      sx.commit(lds + buf * T::BUF + T::GBUF, c0, g.C, PADL - g.pw, tid);
      sx.template load<1>(xn, HW, c0, g.C, tid);
    }
  };
  auto stage_commit = [&](int buf) {
    short* b = lds + buf * T::BUF;
    sg.commit(b, k0, g.K, 0, tid);
    sx.template commit<NPX - 1>(b + T::GBUF, c0, g.C, XAL ? 0 : PADL - g.pw,
                                tid);
  };

  // fragment addresses of k-step 0 (tile row 0, columns 0 .. 31): this
  // wave's 16 channels of x, and go's first 16
  const int px = ((lane >> 4) << 2) + ((lane & 15) >> 2);
  const int aoff = px * STR + ((lane & 3) << 2);
  const int boff = (px + PADL - g.pw) * STR + wid * 16 + ((lane & 3) << 2);

  f32x4 acc[KF][RS];
#pragma unroll
  for (int kf = 0; kf < KF; ++kf)
#pragma unroll
    for (int t = 0; t < RS; ++t) acc[kf][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  stage_load(t_begin);
  stage_middle(0);
  stage_commit(0);
  __syncthreads();

  for (int tl = t_begin; tl < t_end; ++tl) {
    const int buf = (tl - t_begin) & 1;
    const bool more = tl + 1 < t_end;
    if (more) stage_load(tl + 1);
    const short* gb = lds + buf * T::BUF + aoff;
    const short* xb = lds + buf * T::BUF + T::GBUF + boff;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks == KS / 2 && more) stage_middle(buf ^ 1);
      const int row = ks / KPR, col = (ks % KPR) * 32;
      s16x8 a[KF];
#pragma unroll
      for (int kf = 0; kf < KF; ++kf)
        a[kf] = read_tr16(gb + row * GROW + col * STR + kf * 16, 16 * STR);
#pragma unroll
      for (int t = 0; t < RS; ++t) {
        const s16x8 b = read_tr16(
            xb + (row + t / S) * XROW + (col + t % S) * STR, 16 * STR);
#pragma unroll
        for (int kf = 0; kf < KF; ++kf)
          acc[kf][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[kf], b, acc[kf][t], 0, 0, 0);
      }
    }
    if (more) stage_commit(buf ^ 1);
    __syncthreads();
  }

  // D layout of the MFMA: row (lane >> 4)*4 + reg (k), column lane & 15 (c)
  const int c = c0 + wid * 16 + (lane & 15);
#pragma unroll
  for (int kf = 0; kf < KF; ++kf)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = k0 + kf * 16 + ((lane >> 4) << 2) + reg;
      if (k >= g.K || c >= g.C) continue;
      float* dst = gw + ((int64_t)k * g.C + c) * RS;
#pragma unroll
      for (int t = 0; t < RS; ++t) atomicAdd(dst + t, acc[kf][t][reg]);
    }
}

// ---------------------------------------------------------------------------
// Weight gradient, rolling window (header: "tap_bwdw_ring_kernel")
// ---------------------------------------------------------------------------

struct RingGeom {
  int N, C, H, W, K, OH, OW, ph, pw;
  int col_bands;        // bands of TW output columns of one image
  int strips_per_band;  // strips of `rows` output rows of one band
  int rows;             // output rows of a strip: a multiple of TH
  int k_tiles, c_tiles;
};

template <int R, int S, bool NARROW>
struct RingTile {
  using T = Tile<R, S>;
  static constexpr int KB = 32, CB = NARROW ? 32 : 64;  // channels of go, of x
  static constexpr int TH = 2, TW = T::TW;              // pixels of a step
  // a unit is TH rows; step i reads x units i .. i + D and go unit i
  static constexpr int D = (R - 1 + TH - 1) / TH;
  static constexpr int SLOTS = D + 2;                // x units in the ring
  static constexpr int RROWS = SLOTS * TH;           // x rows in the ring
  static constexpr int GSTR = 48;                    // shorts per go pixel
  static constexpr int XSTR = NARROW ? 48 : 80;      // shorts per x pixel
  static constexpr int GROW = TW * GSTR + 64;        // shorts per go row
  static constexpr int XROW = T::PWL * XSTR + 64;    // shorts per x row
  static constexpr int GUNIT = TH * GROW, XUNIT = TH * XROW;
  static constexpr int GRING = 2 * GUNIT;            // go: two units
  static constexpr int LDS_SHORTS = GRING + SLOTS * XUNIT;
  static_assert(TW % 32 == 0, "a k-step is 32 pixels of one row");
  static_assert(D * TH >= R - 1, "the units of a step cover its patch");
  static_assert(LDS_SHORTS * 2 <= 80 * 1024, "two blocks per CU");
};

template <int R, int S, bool NARROW, bool XAL, bool GAL>
__global__ __launch_bounds__(256, 2) void tap_bwdw_ring_kernel(
    const unsigned short* __restrict__ go, const unsigned short* __restrict__ x,
    float* __restrict__ gw, RingGeom g) {
  using T = RingTile<R, S, NARROW>;
  using FT = Tile<R, S>;
  constexpr int RS = R * S, KB = T::KB, CB = T::CB;
  constexpr int TH = T::TH, TW = T::TW, PADL = FT::PADL, D = T::D;
  constexpr int GSTR = T::GSTR, XSTR = T::XSTR, GROW = T::GROW, XROW = T::XROW;
  constexpr int KFW = NARROW ? 1 : 2;    // go fragments of a wave
  constexpr int KPR = TW / 32;           // k-steps (32 pixels) per row
  constexpr int KS = TH * KPR;           // k-steps per step

  __shared__ __attribute__((aligned(16))) short lds[T::LDS_SHORTS];
  short* gring = lds;
  short* xring = lds + T::GRING;

  // block -> (k tile, c tile, strip, band, image); XCD-aware bijective swizzle
  // as in tap_bwdw_kernel: the k and c tiles of a strip are consecutive, so
  // they share an L2
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int xcd = blockIdx.x & 7, sub = blockIdx.x >> 3;
  int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + sub;
  if (bid >= nwg) bid = blockIdx.x;  // never taken: the mapping is bijective
  const int k0 = (bid % g.k_tiles) * KB;
  bid /= g.k_tiles;
  const int c0 = (bid % g.c_tiles) * CB;
  bid /= g.c_tiles;
  const int oh_b = (bid % g.strips_per_band) * g.rows;
  bid /= g.strips_per_band;
  const int ow0 = (bid % g.col_bands) * TW;
  const int n = bid / g.col_bands;
  const int oh_e = oh_b + g.rows < g.OH ? oh_b + g.rows : g.OH;
  const int steps = (oh_e - oh_b + TH - 1) / TH;  // >= 1: oh_b < OH

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int HW = g.H * g.W, OHW = g.OH * g.OW;
  const unsigned short* gon = go + (int64_t)n * g.K * OHW;
  const unsigned short* xn = x + (int64_t)n * g.C * HW;

  // x on the 16-byte path has two register sets: the loads of step i + 2 are
  // issued while those of step i + 1 are still uncommitted. go, and x by
  // elements, are loaded one step ahead into one set: with two the wide
  // instantiations spilled.
  using OpG = Operand<TH, TW, TW, KB / 8, GSTR, GROW, GAL>;
  using OpX = Operand<TH, FT::PWL, FT::PWN, CB / 8, XSTR, XROW, XAL>;
  OpG sg;
  OpX sx0, sx1;
  const int xcol0 = XAL ? ow0 - PADL : ow0 - g.pw;
  const int xlc0 = XAL ? 0 : PADL - g.pw;
  // x unit u of the strip: input rows oh_b - ph + u*TH .. + TH
  auto load_x = [&](OpX& sx, int u) {
    sx.locate(tid, oh_b - g.ph + u * TH, xcol0, g.H, g.W);
    sx.load(xn, HW, c0, g.C, tid);
  };
  // what step d adds to the rings: go unit d (zero below the strip) and x
  // unit d + D
  auto load_g = [&](int d) {
    sg.locate(tid, oh_b + d * TH, ow0, oh_e, g.OW);
    sg.load(gon, OHW, k0, g.K, tid);
  };
  auto commit = [&](OpX& sx, int d, int xslot) {
    sg.commit(gring + (d & 1) * T::GUNIT, k0, g.K, 0, tid);
    sx.commit(xring + xslot * T::XUNIT, c0, g.C, xlc0, tid);
  };

  // fragment addresses of k-step 0 of ring row 0: this wave's channels
  const int kw = NARROW ? (wid & 1) : 0, cw = NARROW ? (wid >> 1) : wid;
  const int px = ((lane >> 4) << 2) + ((lane & 15) >> 2);
  const int aoff = px * GSTR + kw * 16 + ((lane & 3) << 2);
  const int boff = (px + PADL - g.pw) * XSTR + cw * 16 + ((lane & 3) << 2);

  f32x4 acc[KFW][RS];
#pragma unroll
  for (int kf = 0; kf < KFW; ++kf)
#pragma unroll
    for (int t = 0; t < RS; ++t) acc[kf][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fill: the D units above step 0's own, then step 0; step 1 in flight
#pragma unroll
  for (int u = 0; u < D; ++u) {
    load_x(sx0, u);
    sx0.commit(xring + u * T::XUNIT, c0, g.C, xlc0, tid);
  }
  load_g(0);
  load_x(sx0, D);
  commit(sx0, 0, D);
  if (XAL && steps > 1) load_x(sx1, 1 + D);
  __syncthreads();

  int cslot = D + 1;  // ring slot of x unit i + 1 + D
  int base = 0;       // ring row of the step's first patch row
  // step i: x loads of i + 2 into set A (by elements: of i + 1 into set B), go
  // loads of i + 1, MFMAs of i, commit of i + 1 from set B (its slots were
  // last read in step i - 1), one barrier
  auto step = [&](int i, OpX& sxA, OpX& sxB) {
    if (XAL && i + 2 < steps) load_x(sxA, i + 2 + D);
    if (!XAL && i + 1 < steps) load_x(sxB, i + 1 + D);
    if (i + 1 < steps) load_g(i + 1);
    const short* gb = gring + (i & 1) * T::GUNIT + aoff;
    const short* xb = xring + boff;
    int xrow[TH + R - 1];  // patch row q of this step in the ring
#pragma unroll
    for (int q = 0; q < TH + R - 1; ++q) {
      const int r = base + q;
      xrow[q] = (r >= T::RROWS ? r - T::RROWS : r) * XROW;
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int row = ks / KPR, col = (ks % KPR) * 32;
      s16x8 a[KFW];
#pragma unroll
      for (int kf = 0; kf < KFW; ++kf)
        a[kf] = read_tr16(gb + row * GROW + col * GSTR + kf * 16, 16 * GSTR);
#pragma unroll
      for (int t = 0; t < RS; ++t) {
        const s16x8 b = read_tr16(
            xb + xrow[row + t / S] + (col + t % S) * XSTR, 16 * XSTR);
#pragma unroll
        for (int kf = 0; kf < KFW; ++kf)
          acc[kf][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[kf], b, acc[kf][t], 0, 0, 0);
      }
    }
    if (i + 1 < steps) commit(sxB, i + 1, cslot);
    cslot = cslot + 1 == T::SLOTS ? 0 : cslot + 1;
    base = base + TH == T::RROWS ? 0 : base + TH;
    __syncthreads();
  };
  for (int i = 0; i < steps; i += 2) {
    step(i, sx0, sx1);
    if (i + 1 < steps) step(i + 1, sx1, sx0);
  }

  // D layout of the MFMA: row (lane >> 4)*4 + reg (k), column lane & 15 (c)
  const int c = c0 + cw * 16 + (lane & 15);
#pragma unroll
  for (int kf = 0; kf < KFW; ++kf)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = k0 + (kw + kf) * 16 + ((lane >> 4) << 2) + reg;
      if (k >= g.K || c >= g.C) continue;
      float* dst = gw + ((int64_t)k * g.C + c) * RS;
#pragma unroll
      for (int t = 0; t < RS; ++t) atomicAdd(dst + t, acc[kf][t][reg]);
    }
}

// ---------------------------------------------------------------------------
// Weight gradient, pixel-major (header: "tap_bwdw_px_kernel")
// ---------------------------------------------------------------------------

template <int R, int S>
struct PxTile {
  using T = Tile<R, S>;
  static constexpr int KB = 128, CB = 32;        // channels of go, of x
  static constexpr int TH = S == 7 ? 2 : 4;      // 128 pixels a step
  static constexpr int TW = T::TW;
  static constexpr int PH = TH + R - 1;
  static constexpr int PADL = T::PADL, PWL = T::PWL;
  static constexpr int PWC = S / 2;              // the pad of the constant shifts
  // shorts per channel: the pixels, up to an odd number of 16-byte groups
  static constexpr int odd8(int n) { return (((n + 7) / 8) | 1) * 8; }
  static constexpr int GSTR = odd8(TH * TW);
  static constexpr int XSTR = odd8(PH * PWL);
  static constexpr int GBUF = KB * GSTR;
  static constexpr int BUF = GBUF + CB * XSTR;   // one step: go, then x
  static constexpr int LDS_SHORTS = 2 * BUF;
  static_assert(TW % 32 == 0, "a k-step is 32 pixels of one row");
  static_assert(S == 1 || TW + 16 <= PWL, "the last window lies in the patch");
  static_assert(LDS_SHORTS * 2 <= 160 * 1024, "LDS of one CU");
};

// One operand of a step: CH channels x ROWS x COLS pixels of an NCHW image,
// staged as it lies in memory, [channel][row][column], CSTR shorts a channel.
// An item is 8 consecutive pixels of one row of one channel, one
// ds_write_b128; consecutive threads take consecutive groups of a row.
// ALIGNED: one 16-byte load an item, issued by `load` and written by `commit`.
// Otherwise `load` does nothing and `commit` stages item by item: eight 2-byte
// loads with the column clamped into the row, a mask per pixel, the write. No
// prefetch on that path: with its items held across the MFMAs five of the
// eight such instantiations spilled.
template <int CH, int ROWS, int COLS, int CSTR, bool ALIGNED>
struct PxOperand {
  static constexpr int G = COLS / 8;
  static constexpr int ITEMS = CH * ROWS * G;
  static constexpr int PT = (ITEMS + 255) / 256;  // items per thread
  // channels c0 .. c0 + CH of an image of Cmax channels, HW elements each;
  // rows below Hi and columns below Wi are inside
  const unsigned short* img;
  int HW, c0, Cmax, Hi, Wi;
  int soff[ALIGNED ? PT : 1];  // offset in the channel plane; -1: outside
  i32x4 rawv[ALIGNED ? PT : 1];

  static __device__ __forceinline__ void split(int u, int& ch, int& row,
                                               int& col) {
    col = u % G * 8;
    row = u / G % ROWS;
    ch = u / (G * ROWS);
  }
  // clamped below Cmax: always inside the image (32-bit offsets from a uniform
  // base: an image has fewer than 2^31 elements)
  __device__ __forceinline__ const unsigned short* plane(int ch) const {
    return img + (unsigned)((c0 + ch < Cmax ? c0 + ch : Cmax - 1) * HW);
  }

  // (row0, col0): image coordinates of row 0 and column 0 of the step.
  // Nothing is read of the loads before `commit`.
  __device__ __forceinline__ void load(int tid, int row0, int col0) {
    if constexpr (ALIGNED) {
#pragma unroll
      for (int it = 0; it < PT; ++it) {
        if (it * 256 + tid >= ITEMS) continue;
        int ch, row, col;
        split(it * 256 + tid, ch, row, col);
        const int ih = row0 + row, iw = col0 + col;
        // Wi % 8 == 0 and iw % 8 == 0: a group is wholly in or out
        const bool ok = ih >= 0 && ih < Hi && iw >= 0 && iw < Wi;
        soff[it] = ok ? ih * Wi + iw : -1;
        rawv[it] = *(const i32x4*)(plane(ch) + (ok ? soff[it] : 0));
      }
    }
  }

  // pads, borders, the pixel tail and the channel tail become zeros here
  __device__ __forceinline__ void commit(short* buf, int tid, int row0,
                                         int col0) {
    if constexpr (ALIGNED) {
#pragma unroll
      for (int it = 0; it < PT; ++it) {
        if (it * 256 + tid >= ITEMS) continue;
        int ch, row, col;
        split(it * 256 + tid, ch, row, col);
        const int m = soff[it] >= 0 && c0 + ch < Cmax ? -1 : 0;
        i32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = rawv[it][j] & m;
        *(i32x4*)(buf + ch * CSTR + row * COLS + col) = o;
      }
    } else {
#pragma unroll 1
      for (int u = tid; u < ITEMS; u += 256) {
        int ch, row, col;
        split(u, ch, row, col);
        const int ih = row0 + row, iw = col0 + col;
        const bool rok = ih >= 0 && ih < Hi && c0 + ch < Cmax;
        const unsigned short* p = plane(ch) + (ih >= 0 && ih < Hi ? ih * Wi : 0);
        unsigned v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int w = iw + e;
          const unsigned raw = p[w < 0 ? 0 : w < Wi ? w : Wi - 1];
          v[e] = rok && w >= 0 && w < Wi ? raw : 0u;
        }
        i32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (int)(v[2 * j] | (v[2 * j + 1] << 16));
        *(i32x4*)(buf + ch * CSTR + row * COLS + col) = o;
      }
    }
  }
};

template <int R, int S, bool XAL, bool GAL>
__global__ __launch_bounds__(256) void tap_bwdw_px_kernel(
    const unsigned short* __restrict__ go, const unsigned short* __restrict__ x,
    float* __restrict__ gw, RingGeom g) {
  using T = PxTile<R, S>;
  constexpr int RS = R * S, KB = T::KB, CB = T::CB;
  constexpr int TH = T::TH, TW = T::TW, PWL = T::PWL;
  constexpr int GSTR = T::GSTR, XSTR = T::XSTR;
  constexpr int KFW = KB / 64, CF = CB / 16;  // go fragments of a wave, x's
  constexpr int KPR = TW / 32;                // k-steps (32 pixels) per row
  constexpr int KS = TH * KPR;                // k-steps per step

  __shared__ __attribute__((aligned(16))) short lds[T::LDS_SHORTS];

  // block -> (k tile, c tile, strip, band, image); XCD-aware bijective swizzle
  // as in tap_bwdw_ring_kernel: the output tiles of a strip are consecutive, so
  // they share an L2
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int xcd = blockIdx.x & 7, sub = blockIdx.x >> 3;
  int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + sub;
  if (bid >= nwg) bid = blockIdx.x;  // never taken: the mapping is bijective
  const int k0 = (bid % g.k_tiles) * KB;
  bid /= g.k_tiles;
  const int c0 = (bid % g.c_tiles) * CB;
  bid /= g.c_tiles;
  const int oh_b = (bid % g.strips_per_band) * g.rows;
  bid /= g.strips_per_band;
  const int ow0 = (bid % g.col_bands) * TW;
  const int n = bid / g.col_bands;
  const int oh_e = oh_b + g.rows < g.OH ? oh_b + g.rows : g.OH;
  const int steps = (oh_e - oh_b + TH - 1) / TH;  // >= 1: oh_b < OH

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int HW = g.H * g.W, OHW = g.OH * g.OW;
  const unsigned short* gon = go + (int64_t)n * g.K * OHW;
  const unsigned short* xn = x + (int64_t)n * g.C * HW;

  PxOperand<KB, TH, TW, GSTR, GAL> sg{gon, OHW, k0, g.K, oh_e, g.OW};
  PxOperand<CB, T::PH, PWL, XSTR, XAL> sx{xn, HW, c0, g.C, g.H, g.W};
  // patch column 0: PADL left of the band for the pad PWC of the constant
  // shifts; any other pad moves the image under the patch (by elements only).
  // go is zero below the strip (oh_e).
  const int xcol0 = ow0 - T::PADL + T::PWC - g.pw;
  auto stage_load = [&](int i) {
    sg.load(tid, oh_b + i * TH, ow0);
    sx.load(tid, oh_b + i * TH - g.ph, xcol0);
  };
  auto stage_commit = [&](int i) {
    short* b = lds + (i & 1) * T::BUF;
    sg.commit(b, tid, oh_b + i * TH, ow0);
    sx.commit(b + T::GBUF, tid, oh_b + i * TH - g.ph, xcol0);
  };

  // fragment addresses of k-step 0: lane l holds channel (l & 15) of its
  // fragment at pixels 8 * (l >> 4) .. + 8, for x one group left of them
  const int aoff = (wid * KFW * 16 + (lane & 15)) * GSTR + ((lane >> 4) << 3);
  const int boff = (lane & 15) * XSTR + ((lane >> 4) << 3);
  // a wave whose go channels all lie past K stages and waits, nothing else
  const bool live = k0 + wid * KFW * 16 < g.K;

  f32x4 acc[KFW][CF][RS];
#pragma unroll
  for (int kf = 0; kf < KFW; ++kf)
#pragma unroll
    for (int cf = 0; cf < CF; ++cf)
#pragma unroll
      for (int t = 0; t < RS; ++t)
        acc[kf][cf][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  stage_load(0);
  stage_commit(0);
  __syncthreads();

  for (int i = 0; i < steps; ++i) {
    const bool more = i + 1 < steps;
    if (more) stage_load(i + 1);
    const short* gb = lds + (i & 1) * T::BUF + aoff;
    const short* xb = lds + (i & 1) * T::BUF + T::GBUF + boff;
    if (live) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int row = ks / KPR, col = (ks % KPR) * 32;
        s16x8 a[KFW];
#pragma unroll
        for (int kf = 0; kf < KFW; ++kf)
          a[kf] = *(const s16x8*)(gb + kf * 16 * GSTR + row * TW + col);
#pragma unroll
        for (int cf = 0; cf < CF; ++cf)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const short* p = xb + cf * 16 * XSTR + (row + r) * PWL + col;
            if constexpr (S == 1) {
              const s16x8 b = *(const s16x8*)p;
#pragma unroll
              for (int kf = 0; kf < KFW; ++kf)
                acc[kf][cf][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[kf], b, acc[kf][cf][r], 0, 0, 0);
            } else {
              // the 24 pixels around the fragment; tap s starts at element
              // 8 + s - PWC: even, four registers as they are; odd, four
              // v_alignbit
              unsigned d[12];
#pragma unroll
              for (int q = 0; q < 3; ++q) {
                const i32x4 v = *(const i32x4*)(p + q * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) d[q * 4 + j] = (unsigned)v[j];
              }
#pragma unroll
              for (int s = 0; s < S; ++s) {
                constexpr int E0 = 8 - T::PWC;
                const int m = (E0 + s) / 2;
                i32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  o[j] = (int)((E0 + s) % 2 == 0
                                   ? d[m + j]
                                   : __builtin_amdgcn_alignbit(d[m + j + 1],
                                                               d[m + j], 16));
                const s16x8 b = __builtin_bit_cast(s16x8, o);
#pragma unroll
                for (int kf = 0; kf < KFW; ++kf)
                  acc[kf][cf][r * S + s] =
                      __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                          a[kf], b, acc[kf][cf][r * S + s], 0, 0, 0);
              }
            }
          }
      }
    }
    if (more) stage_commit(i + 1);
    __syncthreads();
  }

  // D layout of the MFMA: row (lane >> 4)*4 + reg (k), column lane & 15 (c)
#pragma unroll
  for (int kf = 0; kf < KFW; ++kf)
#pragma unroll
    for (int cf = 0; cf < CF; ++cf) {
      const int c = c0 + cf * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int k = k0 + (wid * KFW + kf) * 16 + ((lane >> 4) << 2) + reg;
        if (k >= g.K || c >= g.C) continue;
        float* dst = gw + ((int64_t)k * g.C + c) * RS;
#pragma unroll
        for (int t = 0; t < RS; ++t) atomicAdd(dst + t, acc[kf][cf][t][reg]);
      }
    }
}

// ---------------------------------------------------------------------------
// Strided (header: "Strided")
// ---------------------------------------------------------------------------

// Geometry of a strided filter shape, shared by the kernels and the host: 1x7
// runs at stride (1, 2), 7x1 at (2, 1), 3x3 at (2, 2). The tile is TH x TW
// output pixels in the forward and TH x TW phase cells (go pixels) in the
// data gradient.
template <int R, int S>
struct Strided {
  static constexpr int SH = R > 1 ? 2 : 1, SW = S > 1 ? 2 : 1;
  static constexpr int TH = R == 7 ? 8 : 4;
  static constexpr int TW = S == 7 ? 64 : 32;
  static constexpr int PADL = S > 1 ? 8 : 0;  // patch columns left of the tile
  // forward: the input patch
  static constexpr int FPH = (TH - 1) * SH + R;
  static constexpr int FPWN = (TW - 1) * SW + S;
  static constexpr int FPWL = (PADL + FPWN + 7) / 8 * 8;
  // data gradient: the go patch; a class walks MR + 1 row and MS + 1 column
  // taps at most, and two classes lie at most one go pixel apart
  static constexpr int MR = (R - 1) / SH, MS = (S - 1) / SW;
  static constexpr int BPH = TH + MR + SH - 1;
  static constexpr int BPWN = TW + MS + SW - 1;
  static constexpr int BPWL = (PADL + BPWN + 7) / 8 * 8;
};

// One 32-channel chunk of a PH x PWL patch of an NCHW image on its way into
// LDS: channel-innermost, PSTR shorts a pixel, in SH x SW phase planes. Patch
// (row pr, column lc) lies in plane (pr % SH, lc % SW) at (pr / SH, lc / SW).
// Loads, v_perm transpose and masks as in tap_fwd_body, which keeps its own
// copy. ALIGNED: an item is (patch row, 8-pixel group, 8-channel group), its
// eight ds_write_b128 go to alternating column planes. Otherwise wave cg
// stages channel group cg, an item is one pixel of the PWN needed columns.
template <int PH, int PWL, int PWN, int SH, int SW, bool ALIGNED>
struct PhasePatch {
  static constexpr int PHP = (PH + SH - 1) / SH, PWP = PWL / SW;
  static constexpr int PLANE = PHP * PWP * PSTR;   // shorts per plane
  static constexpr int PBUF = SH * SW * PLANE;     // shorts per buffer
  static constexpr int G = PWL / 8;
  static constexpr int TASKS = PH * G * 4, PIX = PH * PWN;
  static constexpr int NT = ALIGNED ? (TASKS + 255) / 256 : (PIX + 63) / 64;
  static_assert(PWL % 8 == 0 && 8 % SW == 0, "8-pixel groups split evenly");
  int soff[NT];  // offset in the channel plane; -1: outside the image, zeros
  int sdst[NT];  // LDS short index of the first write; -1: no item
  i32x4 rawv[ALIGNED ? NT : 1][8];
  unsigned raws[ALIGNED ? 1 : NT][8];

  static __device__ __forceinline__ int dst(int pr, int lc) {
    return ((pr % SH) * SW + lc % SW) * PLANE +
           ((pr / SH) * PWP + lc / SW) * PSTR;
  }
  static __device__ __forceinline__ int group(int tid) {
    return ALIGNED ? tid & 3 : tid >> 6;
  }

  // (row0, col0): image coordinates of patch row 0 and patch column 0
  // (ALIGNED: col0 % 8 == 0 and Wi % 8 == 0, a group is wholly in or out);
  // by elements the columns [lc0, lc0 + PWN) are staged
  __device__ __forceinline__ void locate(int tid, int row0, int col0, int lc0,
                                         int Hi, int Wi) {
#pragma unroll
    for (int it = 0; it < NT; ++it) {
      int pr, lc;
      bool live;
      if constexpr (ALIGNED) {
        const int u = (it * 256 + tid) >> 2;
        lc = (u % G) * 8;
        pr = u / G;
        live = it * 256 + tid < TASKS;
      } else {
        const int v = it * 64 + (tid & 63);
        lc = lc0 + v % PWN;
        pr = v / PWN;
        live = v < PIX;
      }
      const int ih = row0 + pr, iw = col0 + lc;
      const bool ok = live && ih >= 0 && ih < Hi && iw >= 0 && iw < Wi;
      soff[it] = ok ? ih * Wi + iw : -1;
      sdst[it] = live ? dst(pr, lc) + group(tid) * 8 : -1;
    }
  }

  // issue the loads of channels c0 .. c0 + 32 (clamped below Cmax and into
  // the plane: always inside the image); nothing reads them before `commit`
  __device__ __forceinline__ void load(const unsigned short* img, int64_t HW,
                                       int c0, int Cmax, int tid) {
#pragma unroll
    for (int it = 0; it < NT; ++it) {
      if (sdst[it] < 0) continue;
      const int off = soff[it] < 0 ? 0 : soff[it];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + group(tid) * 8 + e;
        const unsigned short* p = img + (int64_t)(c < Cmax ? c : Cmax - 1) * HW + off;
        if constexpr (ALIGNED)
          rawv[it][e] = *(const i32x4*)p;
        else
          raws[it][e] = *p;
      }
    }
  }

  // pads, borders and the channel tail become zeros here
  __device__ __forceinline__ void commit(short* pb, int c0, int Cmax, int tid) {
#pragma unroll
    for (int it = 0; it < NT; ++it) {
      if (sdst[it] < 0) continue;
      const unsigned sm = soff[it] < 0 ? 0u : ~0u;
      unsigned cm[4];  // dword j holds channels 2j (low) and 2j + 1
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + group(tid) * 8 + 2 * j;
        cm[j] = sm & ((c < Cmax ? 0xffffu : 0u) | (c + 1 < Cmax ? 0xffff0000u : 0u));
      }
      if constexpr (ALIGNED) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          // 8x8 transpose of 16-bit values: pixel p of channels 2j and 2j+1
          const unsigned sel = (p & 1) ? 0x07060302u : 0x05040100u;
          i32x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            o[j] = (int)(__builtin_amdgcn_perm((unsigned)rawv[it][2 * j + 1][p >> 1],
                                               (unsigned)rawv[it][2 * j][p >> 1],
                                               sel) & cm[j]);
          // the group starts on a multiple of 8 columns: pixel p is in column
          // plane p % SW, p / SW pixels on
          *(i32x4*)(pb + sdst[it] + (p % SW) * PLANE + (p / SW) * PSTR) = o;
        }
      } else {
        i32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = (int)((raws[it][2 * j] | (raws[it][2 * j + 1] << 16)) & cm[j]);
        *(i32x4*)(pb + sdst[it]) = o;
      }
    }
  }
};

// block -> (k tile, column block, row block, image): the XCD-aware bijective
// swizzle of tap_fwd_body
__device__ __forceinline__ void strided_block(const TapGeom& g, int& kt, int& cb,
                                              int& rb, int& n) {
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int xcd = blockIdx.x & 7, sub = blockIdx.x >> 3;
  int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + sub;
  if (bid >= nwg) bid = blockIdx.x;  // never taken: the mapping is bijective
  kt = bid % g.k_tiles;
  bid /= g.k_tiles;
  cb = bid % g.col_blocks;
  bid /= g.col_blocks;
  rb = bid % g.row_blocks;
  n = bid / g.row_blocks;
}

// The [k][pixel] bf16 image in LDS (rows ES shorts apart, EH x EW pixels) to
// out[n][k0 + k][oh0 ..][ow0 ..]: 16-byte row stores where g.vec_out, guarded
// element stores otherwise. item = (k, 8-pixel segment).
template <int KB, int EH, int EW, int ES>
__device__ __forceinline__ void strided_store(const unsigned short* E,
                                              unsigned short* __restrict__ out,
                                              const TapGeom& g, int n, int k0,
                                              int oh0, int ow0, int tid) {
  constexpr int SEGS = EH * EW / 8;
  static_assert(KB * SEGS % 256 == 0, "whole passes");
  const int64_t OHW = (int64_t)g.OH * g.OW;
#pragma unroll 4
  for (int it = 0; it < KB * SEGS / 256; ++it) {
    const int idx = it * 256 + tid;
    const int seg = idx % SEGS, k = idx / SEGS;
    const int kout = k0 + k;
    const int oh = oh0 + seg / (EW / 8), ow = ow0 + (seg % (EW / 8)) * 8;
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

template <int R, int S, int MF, bool ALIGNED>
__global__ __launch_bounds__(256) void tap_strided_fwd_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ Wt,
    const float* __restrict__ bias, unsigned short* __restrict__ out,
    TapGeom g) {
  using T = Strided<R, S>;
  using P = PhasePatch<T::FPH, T::FPWL, T::FPWN, T::SH, T::SW, ALIGNED>;
  constexpr int SH = T::SH, SW = T::SW, TH = T::TH, TW = T::TW;
  constexpr int PADL = T::PADL, PBUF = P::PBUF, RS = R * S;
  constexpr int KB = MF * 16;
  constexpr int FPR = TW / 16;        // fragments per tile row
  constexpr int NF = TH * FPR / 4;    // fragments per wave
  constexpr int ES = TH * TW + 8;     // epilogue row stride
  constexpr int LDS_SHORTS = 2 * PBUF > KB * ES ? 2 * PBUF : KB * ES;
  static_assert(LDS_SHORTS * 2 <= 160 * 1024, "LDS of one CU");

  int kt, cb, rb, n;
  strided_block(g, kt, cb, rb, n);
  const int k0 = kt * KB;
  const int oh0 = rb * TH, ow0 = cb * TW;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  // patch double buffer; the epilogue's [k][pixel] image overlays it
  __shared__ __attribute__((aligned(16))) short lds[LDS_SHORTS];

  const int64_t HW = (int64_t)g.H * g.W;
  const unsigned short* xn = x + (int64_t)n * g.C * HW;
  // patch row pr is input row oh0*SH - ph + pr, patch column lc is input
  // column ow0*SW - PADL + lc
  P st;
  st.locate(tid, oh0 * SH - g.ph, ow0 * SW - PADL, PADL - g.pw, g.H, g.W);

  // weight fragments: as in tap_fwd_body
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

  // B fragment nf of this wave: tile row frow, columns col0 .. col0 + 15: the
  // input pixels (frow*SH + r, (col0 + j)*SW + PADL - pw + s) of the patch,
  // which for one tap lie in one plane, one pixel apart
  int boff[NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const int f = wid * NF + nf;
    const int frow = f / FPR, col0 = (f % FPR) * 16;
    boff[nf] = (frow * P::PWP + col0 + (lane & 15)) * PSTR + ((lane >> 4) << 3);
  }

  f32x4 acc[MF][NF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int chunks = g.Cp / CK;
  s16x8 a_cur[MF], a_nxt[MF];
  st.load(xn, HW, 0, g.C, tid);
  load_a(a_cur, 0, 0);
  st.commit(lds, 0, g.C, tid);
  __syncthreads();

  for (int ch = 0; ch < chunks; ++ch) {
    const bool more = ch + 1 < chunks;
    if (more) st.load(xn, HW, (ch + 1) * CK, g.C, tid);
    const short* pb = lds + (ch & 1) * PBUF;
#pragma unroll
    for (int t = 0; t < RS; ++t) {
      if (t + 1 < RS)
        load_a(a_nxt, t + 1, ch * CK);
      else if (more)
        load_a(a_nxt, 0, (ch + 1) * CK);
      const int toff = P::dst(t / S, PADL - g.pw + t % S);  // uniform
      s16x8 bfrag[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        bfrag[nf] = *(const s16x8*)(pb + boff[nf] + toff);
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_cur[mf], bfrag[nf], acc[mf][nf], 0, 0, 0);
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) a_cur[mf] = a_nxt[mf];
    }
    if (more) st.commit(lds + ((ch & 1) ^ 1) * PBUF, (ch + 1) * CK, g.C, tid);
    __syncthreads();
  }

  // epilogue: bias, round to bf16, [k][pixel] image, row stores. D layout of
  // the MFMA: row (lane >> 4)*4 + reg, column lane & 15.
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
  strided_store<KB, TH, TW, ES>(E, out, g, n, k0, oh0, ow0, tid);
}

// Data gradient by phase decomposition (header: "Strided"). TapGeom holds the
// launch: C the channels of go (the reduction), H x W the extents of go, K the
// channels of gx, OH x OW the extents of gx, ph and pw the forward's pads.
template <int R, int S, int MF, bool ALIGNED>
__global__ __launch_bounds__(256) void tap_strided_bwd_data_kernel(
    const unsigned short* __restrict__ go, const unsigned short* __restrict__ Wt,
    unsigned short* __restrict__ gx, TapGeom g) {
  using T = Strided<R, S>;
  using P = PhasePatch<T::BPH, T::BPWL, T::BPWN, 1, 1, ALIGNED>;
  constexpr int SH = T::SH, SW = T::SW, TH = T::TH, TW = T::TW;
  constexpr int PADL = T::PADL, PWL = T::BPWL, PBUF = P::PBUF;
  constexpr int MR = T::MR, MS = T::MS;
  constexpr int KB = MF * 16;
  constexpr int FPR = TW / 16;
  constexpr int NF = TH * FPR / 4;
  constexpr int EH = TH * SH, EW = TW * SW;  // the tile in gx
  constexpr int ES = EH * EW + 8;
  constexpr int LDS_SHORTS = 2 * PBUF > KB * ES ? 2 * PBUF : KB * ES;
  static_assert(LDS_SHORTS * 2 <= 160 * 1024, "LDS of one CU");

  int kt, cb, rb, n;
  strided_block(g, kt, cb, rb, n);
  const int k0 = kt * KB;
  const int i0 = rb * TH, j0 = cb * TW;  // first phase cell of the tile
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  __shared__ __attribute__((aligned(16))) short lds[LDS_SHORTS];

  const int64_t HW = (int64_t)g.H * g.W;
  const unsigned short* gn = go + (int64_t)n * g.C * HW;
  // Tap class (ra, rb) = (r % SH, s % SW) serves the gx pixels of phase
  // a = (ra - ph) mod SH, b = (rb - pw) mod SW; its tap r = ra + SH*m reads go
  // row i + (a + ph - ra)/SH - m for cell row i, and (a + ph - ra)/SH is qh or
  // qh + 1 with qh = ph / SH. Likewise for columns.
  const int qh = g.ph / SH, qw = g.pw / SW;
  // patch row pr is go row i0 + qh - MR + pr, patch column lc is go column
  // j0 - PADL + lc; by elements the columns from PADL + qw - MS are staged
  P st;
  st.locate(tid, i0 + qh - MR, j0 - PADL, PADL + qw - MS, g.H, g.W);

  const int64_t wplane = (int64_t)g.Kp * g.Cp;
  int64_t wrow[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int row = k0 + mf * 16 + (lane & 15);
    wrow[mf] = (int64_t)(row < g.Kp ? row : g.Kp - 1) * g.Cp + ((lane >> 4) << 3);
  }
  // Wt is the transposed pre-pass: the forward's tap (r, s) is its tap
  // R*S - 1 - (r*S + s)
  auto load_a = [&](s16x8 (&a)[MF], int r, int s, int c0) {
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
      a[mf] = *(const s16x8*)(Wt + (R * S - 1 - (r * S + s)) * wplane +
                              wrow[mf] + c0);
  };

  // B fragment nf: cell row frow, cell columns col0 .. col0 + 15, at the go
  // pixel of m = MR, m' = MS of a class with both offsets qh, qw
  int boff[NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const int f = wid * NF + nf;
    const int frow = f / FPR, col0 = (f % FPR) * 16;
    boff[nf] = (frow * PWL + col0 + (lane & 15) + PADL + qw - MS) * PSTR +
               ((lane >> 4) << 3);
  }
  // per class: its phase and the offset of its go pixels (uniform values)
  int pa[SH], da[SH], pb_[SW], db[SW];
#pragma unroll
  for (int ra = 0; ra < SH; ++ra) {
    pa[ra] = ((ra - g.ph) % SH + SH) % SH;
    da[ra] = (pa[ra] + g.ph - ra) / SH - qh;
  }
#pragma unroll
  for (int rb2 = 0; rb2 < SW; ++rb2) {
    pb_[rb2] = ((rb2 - g.pw) % SW + SW) % SW;
    db[rb2] = (pb_[rb2] + g.pw - rb2) / SW - qw;
  }

  f32x4 acc[SH * SW][MF][NF];
#pragma unroll
  for (int cl = 0; cl < SH * SW; ++cl)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        acc[cl][mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int chunks = g.Cp / CK;
  s16x8 a_cur[MF], a_nxt[MF];
  st.load(gn, HW, 0, g.C, tid);
  load_a(a_cur, 0, 0, 0);
  st.commit(lds, 0, g.C, tid);
  __syncthreads();

  for (int ch = 0; ch < chunks; ++ch) {
    const bool more = ch + 1 < chunks;
    if (more) st.load(gn, HW, (ch + 1) * CK, g.C, tid);
    const short* pb = lds + (ch & 1) * PBUF;
    // the taps class by class; every class has a first tap (SH <= R, SW <= S)
#pragma unroll
    for (int ra = 0; ra < SH; ++ra)
#pragma unroll
      for (int rb2 = 0; rb2 < SW; ++rb2) {
        const int coff = (da[ra] * PWL + db[rb2]) * PSTR;
#pragma unroll
        for (int r = ra; r < R; r += SH)
#pragma unroll
          for (int s = rb2; s < S; s += SW) {
            // the weights of the tap after this one, in walking order
            if (s + SW < S)
              load_a(a_nxt, r, s + SW, ch * CK);
            else if (r + SH < R)
              load_a(a_nxt, r + SH, rb2, ch * CK);
            else if (rb2 + 1 < SW)
              load_a(a_nxt, ra, rb2 + 1, ch * CK);
            else if (ra + 1 < SH)
              load_a(a_nxt, ra + 1, 0, ch * CK);
            else if (more)
              load_a(a_nxt, 0, 0, (ch + 1) * CK);
            const int toff =
                coff + ((MR - r / SH) * PWL + MS - s / SW) * PSTR;
            s16x8 bfrag[NF];
#pragma unroll
            for (int nf = 0; nf < NF; ++nf)
              bfrag[nf] = *(const s16x8*)(pb + boff[nf] + toff);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
#pragma unroll
              for (int nf = 0; nf < NF; ++nf)
                acc[ra * SW + rb2][mf][nf] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a_cur[mf], bfrag[nf], acc[ra * SW + rb2][mf][nf], 0, 0,
                        0);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) a_cur[mf] = a_nxt[mf];
          }
      }
    if (more) st.commit(lds + ((ch & 1) ^ 1) * PBUF, (ch + 1) * CK, g.C, tid);
    __syncthreads();
  }

  // epilogue: the classes interleaved in the [c][pixel] image of the EH x EW
  // gx tile: cell (row, col) of phase (a, b) is pixel (row*SH + a, col*SW + b)
  unsigned short* E = (unsigned short*)lds;
#pragma unroll
  for (int ra = 0; ra < SH; ++ra)
#pragma unroll
    for (int rb2 = 0; rb2 < SW; ++rb2)
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int k = mf * 16 + ((lane >> 4) << 2) + reg;
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) {
            const int f = wid * NF + nf;
            const int pix = ((f / FPR) * SH + pa[ra]) * EW +
                            ((f % FPR) * 16 + (lane & 15)) * SW + pb_[rb2];
            E[k * ES + pix] = (unsigned short)(
                pack_bf16(acc[ra * SW + rb2][mf][nf][reg], 0.f) & 0xffff);
          }
        }
  __syncthreads();
  strided_store<KB, EH, EW, ES>(E, gx, g, n, k0, i0 * SH, j0 * SW, tid);
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
                          int64_t R, int64_t S, int64_t ph, int64_t pw,
                          const char* who = "tap_fwd") {
  TORCH_CHECK((R == 1 && S == 7) || (R == 7 && S == 1) || (R == 3 && S == 3),
              who, ": kernel size must be 1x7, 7x1 or 3x3 (stride 1, "
              "dilation 1, groups 1), got ", R, "x", S);
  TORCH_CHECK(N >= 1 && C >= 1 && K >= 1 && H >= 1 && W >= 1,
              who, ": N, C, K, H, W must be positive");
  TORCH_CHECK(ph >= 0 && ph <= R - 1 && pw >= 0 && pw <= S - 1,
              who, ": padding must lie in [0, R-1] x [0, S-1], got (", ph,
              ", ", pw, ") for ", R, "x", S);
  TORCH_CHECK(H + 2 * ph >= R && W + 2 * pw >= S,
              who, ": the padded input is smaller than the filter");
  TORCH_CHECK(H * W < (1LL << 30) && C < (1LL << 24) && K < (1LL << 24),
              who, ": problem too large");
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
  g.sc = 1;
  return g;
}

std::string tap_kernel_name(int64_t C, int64_t K, int64_t H, int64_t W,
                            int64_t R, int64_t S, int64_t ph, int64_t pw) {
  check_problem(1, C, K, H, W, R, S, ph, pw);
  return choose((int)K, (int)W, (int)R, (int)S, true).label;
}

// ---- split channels ---------------------------------------------------------

using SplitKern = void (*)(const unsigned short*, const unsigned short*,
                           float*, TapGeom);
constexpr int SPLIT_MAX = 8;  // slices of a launch at most

// MF of a split launch: the unsplit chooser's, but 4 where that is 7 (header)
static int split_mf(int K) { return std::min(choose_mf(K), 4); }

template <int R, int S>
static TapChoice choose_split_rs(int mf, bool aligned, SplitKern& kern) {
  using T = Tile<R, S>;
  if (mf == 2)
    kern = aligned ? tap_fwd_split_kernel<R, S, 2, true>
                   : tap_fwd_split_kernel<R, S, 2, false>;
  else
    kern = aligned ? tap_fwd_split_kernel<R, S, 4, true>
                   : tap_fwd_split_kernel<R, S, 4, false>;
  return {nullptr, mf, T::TH, T::TW,
          "tap_split<" + std::to_string(R) + "x" + std::to_string(S) + "," +
              std::to_string(mf) + ">"};
}

static TapChoice choose_split(int mf, int W, int R, int S, bool base_aligned,
                              SplitKern& kern) {
  const bool aligned = base_aligned && W % 8 == 0;
  if (R == 1 && S == 7) return choose_split_rs<1, 7>(mf, aligned, kern);
  if (R == 7 && S == 1) return choose_split_rs<7, 1>(mf, aligned, kern);
  return choose_split_rs<3, 3>(mf, aligned, kern);
}

// (MF, SC) of a problem on a device of `cus` compute units: the one place that
// decides whether and how far the channels are split (rule: file header).
// SC == 1: the unsplit kernel with the unsplit chooser's MF.
std::pair<int, int> tap_split_choice(int64_t N, int64_t C, int64_t K,
                                     int64_t H, int64_t W, int64_t R,
                                     int64_t S, int64_t ph, int64_t pw,
                                     int64_t cus) {
  const TapChoice un = choose((int)K, (int)W, (int)R, (int)S, true);
  const int64_t OH = H + 2 * ph - R + 1, OW = W + 2 * pw - S + 1;
  const int64_t tiles =
      N * ((OH + un.th - 1) / un.th) * ((OW + un.tw - 1) / un.tw);
  auto k_tiles = [&](int mf) { return (K + mf * 16 - 1) / (mf * 16); };
  if (k_tiles(un.mf) * tiles >= 2 * cus) return {un.mf, 1};
  const int mf = split_mf((int)K);
  const int64_t cap = std::min<int64_t>((C + CK - 1) / CK, SPLIT_MAX);
  int64_t sc = 1;
  while (sc < cap && k_tiles(mf) * tiles * sc < 2 * cus) ++sc;
  if (sc == 1) return {un.mf, 1};
  return {mf, (int)sc};
}

std::pair<std::string, int64_t> tap_split_kernel_name(
    int64_t N, int64_t C, int64_t K, int64_t H, int64_t W, int64_t R,
    int64_t S, int64_t ph, int64_t pw, int64_t cus) {
  check_problem(N, C, K, H, W, R, S, ph, pw, "tap_split_kernel_name");
  TORCH_CHECK(cus >= 1, "tap_split_kernel_name: cus must be positive");
  const auto [mf, sc] = tap_split_choice(N, C, K, H, W, R, S, ph, pw, cus);
  if (sc == 1) return {choose((int)K, (int)W, (int)R, (int)S, true).label, 1};
  SplitKern kern;
  return {choose_split(mf, (int)W, (int)R, (int)S, true, kern).label, sc};
}

torch::Tensor tap_fwd(torch::Tensor x, torch::Tensor w,
                      c10::optional<torch::Tensor> bias, int64_t ph, int64_t pw,
                      bool transposed, int64_t split) {
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
  // split: 0 the unsplit kernel, -1 the chooser's slices, n > 0 n slices
  const int64_t chunks = (Cred + CK - 1) / CK;
  TORCH_CHECK(split >= -1, "tap_fwd: split must be -1, 0 or a slice count");
  TORCH_CHECK(split <= chunks, "tap_fwd: split = ", split, " slices, but C = ",
              Cred, " has only ", chunks, " chunks of ", CK, " channels");
  TORCH_CHECK(split <= SPLIT_MAX, "tap_fwd: split = ", split,
              " slices, at most ", SPLIT_MAX, " are supported");
  int sc = (int)split, smf = split_mf((int)Kout);
  if (split < 0) {
    const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    std::tie(smf, sc) = tap_split_choice(x.size(0), Cred, Kout, x.size(2),
                                         x.size(3), R, S, ph, pw, cus);
  }
  SplitKern skern = nullptr;
  const TapChoice ch =
      sc > 1 ? choose_split(smf, (int)x.size(3), (int)R, (int)S, base_aligned,
                            skern)
             : choose((int)Kout, (int)x.size(3), (int)R, (int)S, base_aligned);
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
      (int64_t)g.k_tiles * g.row_blocks * g.col_blocks * g.N * std::max(sc, 1);
  TORCH_CHECK(fblocks < (1LL << 31) && blocks < (1LL << 31),
              "tap_fwd: grid too large");
  hipLaunchKernelGGL(tap_filter_kernel, dim3((uint32_t)fblocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)w.data_ptr(),
                     (unsigned short*)Wt.data_ptr(), (int)Cw, g.K, g.C, g.Kp,
                     g.Cp, (int)(R * S), transposed ? 1 : 0);
  if (sc <= 1) {
    hipLaunchKernelGGL(ch.kern, dim3((uint32_t)blocks), dim3(256), 0,
                       stream.stream(), (const unsigned short*)x.data_ptr(),
                       (const unsigned short*)Wt.data_ptr(), bptr,
                       (unsigned short*)out.data_ptr(), g);
    return out;
  }
  // split: partial sums of the slices, then their sum, the bias and rounding
  const int64_t OHW = (int64_t)g.OH * g.OW, total = out.numel();
  auto part = torch::empty({sc, g.N, g.K, g.OH, g.OW},
                           x.options().dtype(torch::kFloat));
  const bool part_al = ((uintptr_t)part.data_ptr() & 15) == 0;
  const bool vec_red = OHW % 8 == 0 && part_al &&
                       ((uintptr_t)out.data_ptr() & 15) == 0;
  const int64_t rblocks = (total / (vec_red ? 8 : 1) + 255) / 256;
  TORCH_CHECK(rblocks < (1LL << 31), "tap_fwd: grid too large");
  g.sc = sc;
  g.vec_out = g.OW % 4 == 0 && part_al;  // 16 bytes are four fp32 here
  hipLaunchKernelGGL(skern, dim3((uint32_t)blocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)x.data_ptr(),
                     (const unsigned short*)Wt.data_ptr(),
                     part.data_ptr<float>(), g);
  hipLaunchKernelGGL(vec_red ? tap_split_reduce_kernel<true>
                             : tap_split_reduce_kernel<false>,
                     dim3((uint32_t)rblocks), dim3(256), 0, stream.stream(),
                     (const float*)part.data_ptr<float>(), bptr,
                     (unsigned short*)out.data_ptr(), sc, g.K, OHW, total);
  return out;
}

// ---- strided ----------------------------------------------------------------

using BwdKern = void (*)(const unsigned short*, const unsigned short*,
                         unsigned short*, TapGeom);

// The instantiation of a strided problem: the only place that decides MF and
// ALIGNED. Forward: the stride-1 chooser's MF. Data gradient: the same, but at
// most 4 for 3x3, whose four classes hold 4 * MF * 2 accumulator fragments.
struct StridedChoice {
  Kern fwd;
  BwdKern bwd;
  int mf, th, tw, sh, sw;
  std::string label;
};

template <int R, int S, int MF>
static void strided_kernels(StridedChoice& c, bool aligned) {
  c.fwd = aligned ? tap_strided_fwd_kernel<R, S, MF, true>
                  : tap_strided_fwd_kernel<R, S, MF, false>;
  c.bwd = aligned ? tap_strided_bwd_data_kernel<R, S, MF, true>
                  : tap_strided_bwd_data_kernel<R, S, MF, false>;
}

template <int R, int S>
static StridedChoice choose_strided_rs(int mf, bool transposed, bool aligned) {
  using T = Strided<R, S>;
  if (transposed && R == 3 && mf > 4) mf = 4;
  StridedChoice c{nullptr, nullptr, mf, T::TH, T::TW, T::SH, T::SW,
                  std::string(transposed ? "tap_strided_bwd<" : "tap_strided<") +
                      std::to_string(R) + "x" + std::to_string(S) + "," +
                      std::to_string(mf) + ">"};
  if (mf == 2)
    strided_kernels<R, S, 2>(c, aligned);
  else if (mf == 4)
    strided_kernels<R, S, 4>(c, aligned);
  else if constexpr (R != 3)
    strided_kernels<R, S, 7>(c, aligned);
  else  // 3x3 forward only
    c.fwd = aligned ? tap_strided_fwd_kernel<R, S, 7, true>
                    : tap_strided_fwd_kernel<R, S, 7, false>;
  return c;
}

// Kout: the output channels of the launch; Wst: the row length of the image
// the launch stages (x, or go for the data gradient)
static StridedChoice choose_strided(int Kout, int Wst, int R, int S,
                                    bool transposed, bool base_aligned) {
  const int mf = choose_mf(Kout);
  const bool aligned = base_aligned && Wst % 8 == 0;
  if (R == 1 && S == 7) return choose_strided_rs<1, 7>(mf, transposed, aligned);
  if (R == 7 && S == 1) return choose_strided_rs<7, 1>(mf, transposed, aligned);
  return choose_strided_rs<3, 3>(mf, transposed, aligned);
}

// (N, C, K, H, W): the forward convolution's, whichever leg is asked for
static void check_strided(int64_t N, int64_t C, int64_t K, int64_t H, int64_t W,
                          int64_t R, int64_t S, int64_t sh, int64_t sw,
                          int64_t ph, int64_t pw, const char* who) {
  TORCH_CHECK((R == 1 && S == 7) || (R == 7 && S == 1) || (R == 3 && S == 3),
              who, ": kernel size must be 1x7, 7x1 or 3x3 (dilation 1, "
              "groups 1), got ", R, "x", S);
  TORCH_CHECK(sh == (R > 1 ? 2 : 1) && sw == (S > 1 ? 2 : 1),
              who, ": stride must be (1, 2) for 1x7, (2, 1) for 7x1 and "
              "(2, 2) for 3x3, got (", sh, ", ", sw, ") for ", R, "x", S);
  TORCH_CHECK(N >= 1 && C >= 1 && K >= 1 && H >= 1 && W >= 1,
              who, ": N, C, K, H, W must be positive");
  TORCH_CHECK(ph >= 0 && ph <= R - 1 && pw >= 0 && pw <= S - 1,
              who, ": padding must lie in [0, R-1] x [0, S-1], got (", ph,
              ", ", pw, ") for ", R, "x", S);
  TORCH_CHECK(H + 2 * ph >= R && W + 2 * pw >= S,
              who, ": the padded input is smaller than the filter");
  TORCH_CHECK(H * W < (1LL << 30) && C < (1LL << 24) && K < (1LL << 24),
              who, ": problem too large");
}

// transposed: C the reduction dim and K the output channels of the launch (the
// forward's K and C); H x W the forward's input in both cases
std::string tap_strided_kernel_name(int64_t C, int64_t K, int64_t H, int64_t W,
                                    int64_t R, int64_t S, int64_t sh,
                                    int64_t sw, int64_t ph, int64_t pw,
                                    bool transposed) {
  check_strided(1, transposed ? K : C, transposed ? C : K, H, W, R, S, sh, sw,
                ph, pw, "tap_strided_kernel_name");
  const int64_t OW = (W + 2 * pw - S) / sw + 1;
  return choose_strided((int)K, (int)(transposed ? OW : W), (int)R, (int)S,
                        transposed, true).label;
}

static void check_strided_tensors(const torch::Tensor& a, const torch::Tensor& w,
                                  const char* who) {
  TORCH_CHECK(a.is_cuda() && w.is_cuda() && a.get_device() == w.get_device(),
              who, ": the tensors must be on one GPU");
  TORCH_CHECK(a.dim() == 4 && w.dim() == 4 && a.is_contiguous() &&
                  w.is_contiguous(),
              who, ": the tensors must be contiguous and 4-d");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
                  w.scalar_type() == torch::kBFloat16,
              who, ": bf16 only");
}

// The pre-pass and the main kernel of either leg. g.C / g.K: the reduction and
// output channels of the launch; src: the staged image, dst: the result.
static void launch_strided(const StridedChoice& ch, TapGeom g,
                           const torch::Tensor& src, const torch::Tensor& w,
                           const float* bias, torch::Tensor& dst,
                           bool transposed, const char* who) {
  const int64_t RS = w.size(2) * w.size(3);
  g.Kp = (g.K + 15) / 16 * 16;
  g.Cp = (g.C + CK - 1) / CK * CK;
  g.k_tiles = (g.K + ch.mf * 16 - 1) / (ch.mf * 16);
  g.vec_out = g.OW % 8 == 0 && ((uintptr_t)dst.data_ptr() & 15) == 0;
  g.sc = 1;
  auto Wt = torch::empty({RS, g.Kp, g.Cp}, src.options());
  const int64_t fblocks = ((int64_t)g.Kp * g.Cp + 255) / 256;
  const int64_t blocks =
      (int64_t)g.k_tiles * g.row_blocks * g.col_blocks * g.N;
  TORCH_CHECK(fblocks < (1LL << 31) && blocks < (1LL << 31), who,
              ": grid too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(tap_filter_kernel, dim3((uint32_t)fblocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)w.data_ptr(),
                     (unsigned short*)Wt.data_ptr(), (int)w.size(1), g.K, g.C,
                     g.Kp, g.Cp, (int)RS, transposed ? 1 : 0);
  if (transposed)
    hipLaunchKernelGGL(ch.bwd, dim3((uint32_t)blocks), dim3(256), 0,
                       stream.stream(), (const unsigned short*)src.data_ptr(),
                       (const unsigned short*)Wt.data_ptr(),
                       (unsigned short*)dst.data_ptr(), g);
  else
    hipLaunchKernelGGL(ch.fwd, dim3((uint32_t)blocks), dim3(256), 0,
                       stream.stream(), (const unsigned short*)src.data_ptr(),
                       (const unsigned short*)Wt.data_ptr(), bias,
                       (unsigned short*)dst.data_ptr(), g);
}

torch::Tensor tap_fwd_strided(torch::Tensor x, torch::Tensor w,
                              c10::optional<torch::Tensor> bias, int64_t sh,
                              int64_t sw, int64_t ph, int64_t pw) {
  const char* who = "tap_fwd_strided";
  check_strided_tensors(x, w, who);
  const int64_t K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  check_strided(x.size(0), C, K, x.size(2), x.size(3), R, S, sh, sw, ph, pw,
                who);
  TORCH_CHECK(x.size(1) == C, who, ": channel mismatch: x has ", x.size(1),
              ", the filter reduces over ", C);
  const StridedChoice ch =
      choose_strided((int)K, (int)x.size(3), (int)R, (int)S, false,
                     ((uintptr_t)x.data_ptr() & 15) == 0);
  TapGeom g;
  g.N = (int)x.size(0); g.C = (int)C; g.K = (int)K;
  g.H = (int)x.size(2); g.W = (int)x.size(3);
  g.ph = (int)ph; g.pw = (int)pw;
  g.OH = (g.H + 2 * g.ph - (int)R) / ch.sh + 1;
  g.OW = (g.W + 2 * g.pw - (int)S) / ch.sw + 1;
  g.row_blocks = (g.OH + ch.th - 1) / ch.th;
  g.col_blocks = (g.OW + ch.tw - 1) / ch.tw;
  const float* bptr = nullptr;
  torch::Tensor b32;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->get_device() == x.get_device() &&
                    bias->numel() == K,
                who, ": bias must hold one value per output channel, on x's GPU");
    b32 = bias->to(torch::kFloat).contiguous();
    bptr = b32.data_ptr<float>();
  }
  auto out = torch::empty({g.N, g.K, g.OH, g.OW}, x.options());
  launch_strided(ch, g, x, w, bptr, out, false, who);
  return out;
}

torch::Tensor tap_bwd_data_strided(torch::Tensor go, torch::Tensor w, int64_t H,
                                   int64_t W, int64_t sh, int64_t sw,
                                   int64_t ph, int64_t pw) {
  const char* who = "tap_bwd_data_strided";
  check_strided_tensors(go, w, who);
  const int64_t K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  check_strided(go.size(0), C, K, H, W, R, S, sh, sw, ph, pw, who);
  const int64_t OH = (H + 2 * ph - R) / sh + 1, OW = (W + 2 * pw - S) / sw + 1;
  TORCH_CHECK(go.size(1) == K && go.size(2) == OH && go.size(3) == OW, who,
              ": go must be [N, ", K, ", ", OH, ", ", OW, "] for an input of ",
              H, " x ", W);
  const StridedChoice ch =
      choose_strided((int)C, (int)OW, (int)R, (int)S, true,
                     ((uintptr_t)go.data_ptr() & 15) == 0);
  // the launch stages go and reduces over its channels; a block owns th x tw
  // phase cells, that is (th*sh) x (tw*sw) pixels of gx
  TapGeom g;
  g.N = (int)go.size(0); g.C = (int)K; g.K = (int)C;
  g.H = (int)OH; g.W = (int)OW;
  g.ph = (int)ph; g.pw = (int)pw;
  g.OH = (int)H; g.OW = (int)W;
  g.row_blocks = ((g.OH + ch.sh - 1) / ch.sh + ch.th - 1) / ch.th;
  g.col_blocks = ((g.OW + ch.sw - 1) / ch.sw + ch.tw - 1) / ch.tw;
  auto gx = torch::empty({g.N, g.K, g.OH, g.OW}, go.options());
  launch_strided(ch, g, go, w, nullptr, gx, true, who);
  return gx;
}

// ---- weight gradient --------------------------------------------------------

using WgKern = void (*)(const unsigned short*, const unsigned short*, float*,
                        WgGeom);

// The launch of a weight-gradient problem: the only place that decides the
// instantiation, the run length and the grid.
struct WgChoice {
  WgKern kern;
  WgGeom g;
  int64_t blocks;
  std::string label;
};

template <int R, int S>
static WgChoice choose_bwdw_rs(WgGeom g, bool xal, bool gal,
                               int64_t tiles_per_block) {
  using T = WgTile<R, S>;
  constexpr int CUS = 256;
  g.row_blocks = (g.OH + T::TH - 1) / T::TH;
  g.col_blocks = (g.OW + T::TW - 1) / T::TW;
  const int64_t tiles = (int64_t)g.N * g.row_blocks * g.col_blocks;
  TORCH_CHECK(tiles < (1LL << 31), "tap_bwd_weight: problem too large");
  g.tiles = (int)tiles;
  g.k_tiles = (g.K + T::KF * 16 - 1) / (T::KF * 16);
  g.c_tiles = (g.C + T::CF * 16 - 1) / (T::CF * 16);
  // about two blocks per CU; at least one per CU where there are that many
  // (output tile, pixel tile) pairs
  const int64_t ot = (int64_t)g.k_tiles * g.c_tiles;
  int64_t tpb = tiles_per_block;
  if (tpb <= 0) {
    const int64_t runs = std::max<int64_t>(1, 2 * CUS / ot);
    // where tiles >= runs, ceil(tiles / tpb) > runs / 2, so the grid has at
    // least ot * (runs + 1) / 2 > CUS blocks; with fewer tiles tpb is 1 and
    // the grid is every (output tile, pixel tile) pair
    tpb = (tiles + runs - 1) / runs;
  }
  tpb = std::min<int64_t>(tpb, tiles);
  g.tpb = (int)tpb;
  const int64_t blocks = ot * ((tiles + tpb - 1) / tpb);
  const WgKern k = xal ? (gal ? tap_bwdw_kernel<R, S, true, true>
                              : tap_bwdw_kernel<R, S, true, false>)
                       : (gal ? tap_bwdw_kernel<R, S, false, true>
                              : tap_bwdw_kernel<R, S, false, false>);
  return {k, g, blocks,
          "tap_bwdw<" + std::to_string(R) + "x" + std::to_string(S) + "," +
              std::to_string(T::KF * 16) + "x" + std::to_string(T::CF * 16) +
              ",tpb" + std::to_string(tpb) + ">"};
}

static WgChoice choose_bwdw(int64_t N, int64_t C, int64_t K, int64_t H,
                            int64_t W, int64_t R, int64_t S, int64_t ph,
                            int64_t pw, bool x_aligned, bool go_aligned,
                            int64_t tiles_per_block) {
  check_problem(N, C, K, H, W, R, S, ph, pw, "tap_bwd_weight");
  WgGeom g;
  g.N = (int)N; g.C = (int)C; g.K = (int)K; g.H = (int)H; g.W = (int)W;
  g.ph = (int)ph; g.pw = (int)pw;
  g.OH = g.H + 2 * g.ph - (int)R + 1;
  g.OW = g.W + 2 * g.pw - (int)S + 1;
  // the kernel addresses one image of x and of go with 32-bit offsets
  TORCH_CHECK(C * H * W < (1LL << 31) && K * g.OH * g.OW < (1LL << 31),
              "tap_bwd_weight: problem too large");
  const bool xal = x_aligned && g.W % 8 == 0;
  const bool gal = go_aligned && g.OW % 8 == 0;
  if (R == 1) return choose_bwdw_rs<1, 7>(g, xal, gal, tiles_per_block);
  if (R == 7) return choose_bwdw_rs<7, 1>(g, xal, gal, tiles_per_block);
  return choose_bwdw_rs<3, 3>(g, xal, gal, tiles_per_block);
}

std::string tap_bwdw_kernel_name(int64_t N, int64_t C, int64_t K, int64_t H,
                                 int64_t W, int64_t R, int64_t S, int64_t ph,
                                 int64_t pw) {
  return choose_bwdw(N, C, K, H, W, R, S, ph, pw, true, true, 0).label;
}

// gw[k][c][r][s] += sum over n, oh, ow of go[n][k][oh][ow] *
// x[n][c][oh-ph+r][ow-pw+s]. With `out` (fp32, contiguous, K*C*R*S elements,
// go's device) the kernel's atomicAdd accumulates into it; without, into a
// fresh zeroed tensor: conv_bwd_weight's contract.
torch::Tensor tap_bwd_weight(torch::Tensor go, torch::Tensor x, int64_t R,
                             int64_t S, int64_t ph, int64_t pw,
                             c10::optional<torch::Tensor> out,
                             int64_t tiles_per_block) {
  TORCH_CHECK(go.is_cuda() && x.is_cuda() && go.get_device() == x.get_device(),
              "tap_bwd_weight: go and x must be on one GPU");
  TORCH_CHECK(go.dim() == 4 && x.dim() == 4 && go.is_contiguous() &&
                  x.is_contiguous(),
              "tap_bwd_weight: go and x must be contiguous 4-d tensors");
  TORCH_CHECK(go.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              "tap_bwd_weight: bf16 only");
  const WgChoice ch = choose_bwdw(
      x.size(0), x.size(1), go.size(1), x.size(2), x.size(3), R, S, ph, pw,
      ((uintptr_t)x.data_ptr() & 15) == 0, ((uintptr_t)go.data_ptr() & 15) == 0,
      tiles_per_block);
  const WgGeom& g = ch.g;
  TORCH_CHECK(go.size(0) == g.N && go.size(2) == g.OH && go.size(3) == g.OW,
              "tap_bwd_weight: go is not the gradient of this convolution");
  const int64_t numel = (int64_t)g.K * g.C * R * S;
  torch::Tensor gw;
  if (out.has_value()) {
    gw = *out;
    TORCH_CHECK(gw.is_cuda() && gw.get_device() == go.get_device() &&
                    gw.scalar_type() == torch::kFloat && gw.is_contiguous() &&
                    gw.numel() == numel,
                "tap_bwd_weight: out must be a contiguous fp32 tensor of "
                "K*C*R*S elements on go's device");
  } else {
    gw = torch::zeros({numel}, x.options().dtype(torch::kFloat));
  }
  TORCH_CHECK(ch.blocks < (1LL << 31), "tap_bwd_weight: grid too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(ch.kern, dim3((uint32_t)ch.blocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)go.data_ptr(),
                     (const unsigned short*)x.data_ptr(), gw.data_ptr<float>(),
                     g);
  return gw.view({(int64_t)g.K, (int64_t)g.C, R, S});
}

// ---- weight gradient, rolling window ----------------------------------------

using RingKern = void (*)(const unsigned short*, const unsigned short*, float*,
                          RingGeom);

// The launch of a rolling-window problem: the only place that decides the
// instantiation, the strip length and the grid.
struct RingChoice {
  RingKern kern;
  RingGeom g;
  int64_t blocks;
  std::string label;
};

template <int R, int S, bool NARROW>
static RingChoice choose_ring_rs(RingGeom g, bool xal, bool gal,
                                 int64_t strip_rows) {
  using T = RingTile<R, S, NARROW>;
  constexpr int64_t GRID = 4 * 256;  // two resident blocks per CU, two rounds
  g.col_bands = (g.OW + T::TW - 1) / T::TW;
  g.k_tiles = (g.K + T::KB - 1) / T::KB;
  g.c_tiles = (g.C + T::CB - 1) / T::CB;
  const int64_t ot = (int64_t)g.k_tiles * g.c_tiles;
  const int64_t bands = (int64_t)g.N * g.col_bands;
  const int64_t row_steps = (g.OH + T::TH - 1) / T::TH;  // steps of one band
  // `need` strips a band make ot * bands * need >= GRID blocks. With
  // spb = floor(row_steps / need) steps a strip, a band has
  // ceil(row_steps / spb) >= need strips wherever row_steps >= need; with
  // fewer steps spb is 1 and the grid is every (output tile, step) pair.
  int64_t spb = (strip_rows + T::TH - 1) / T::TH;
  if (strip_rows <= 0) {
    const int64_t need = (GRID + ot * bands - 1) / (ot * bands);
    spb = row_steps / need;
  }
  spb = std::min(std::max<int64_t>(spb, 1), row_steps);
  g.rows = (int)(spb * T::TH);
  g.strips_per_band = (int)((row_steps + spb - 1) / spb);
  const int64_t blocks = ot * bands * g.strips_per_band;
  RingKern k = gal ? tap_bwdw_ring_kernel<R, S, NARROW, true, true>
                   : tap_bwdw_ring_kernel<R, S, NARROW, true, false>;
  if constexpr (NARROW) {  // the wide tile is built for the 16-byte x path only
    if (!xal)
      k = gal ? tap_bwdw_ring_kernel<R, S, true, false, true>
              : tap_bwdw_ring_kernel<R, S, true, false, false>;
  } else {
    TORCH_INTERNAL_ASSERT(xal);  // choose_ring sends x by elements to NARROW
  }
  return {k, g, blocks,
          "tap_bwdw_ring<" + std::to_string(R) + "x" + std::to_string(S) + "," +
              std::to_string(T::KB) + "x" + std::to_string(T::CB) + ",rows" +
              std::to_string(g.rows) + ">"};
}

static RingChoice choose_ring(int64_t N, int64_t C, int64_t K, int64_t H,
                              int64_t W, int64_t R, int64_t S, int64_t ph,
                              int64_t pw, bool x_aligned, bool go_aligned,
                              int64_t strip_rows) {
  check_problem(N, C, K, H, W, R, S, ph, pw, "tap_bwd_weight_ring");
  RingGeom g;
  g.N = (int)N; g.C = (int)C; g.K = (int)K; g.H = (int)H; g.W = (int)W;
  g.ph = (int)ph; g.pw = (int)pw;
  g.OH = g.H + 2 * g.ph - (int)R + 1;
  g.OW = g.W + 2 * g.pw - (int)S + 1;
  // the kernel addresses one image of x and of go with 32-bit offsets
  TORCH_CHECK(C * H * W < (1LL << 31) && K * g.OH * g.OW < (1LL << 31),
              "tap_bwd_weight_ring: problem too large");
  const bool xal = x_aligned && g.W % 8 == 0;
  const bool gal = go_aligned && g.OW % 8 == 0;
  // the 32-channel c tile where it pads fewer channels than the 64 tile, and
  // wherever x is staged by elements: the wide tile spilled there
  const bool narrow = !xal || (C + 31) / 32 * 32 < (C + 63) / 64 * 64;
  if (R == 1)
    return narrow ? choose_ring_rs<1, 7, true>(g, xal, gal, strip_rows)
                  : choose_ring_rs<1, 7, false>(g, xal, gal, strip_rows);
  if (R == 7)
    return narrow ? choose_ring_rs<7, 1, true>(g, xal, gal, strip_rows)
                  : choose_ring_rs<7, 1, false>(g, xal, gal, strip_rows);
  return narrow ? choose_ring_rs<3, 3, true>(g, xal, gal, strip_rows)
                : choose_ring_rs<3, 3, false>(g, xal, gal, strip_rows);
}

std::string tap_bwdw_ring_kernel_name(int64_t N, int64_t C, int64_t K,
                                      int64_t H, int64_t W, int64_t R,
                                      int64_t S, int64_t ph, int64_t pw) {
  return choose_ring(N, C, K, H, W, R, S, ph, pw, true, true, 0).label;
}

// tap_bwd_weight's contract on tap_bwdw_ring_kernel.
torch::Tensor tap_bwd_weight_ring(torch::Tensor go, torch::Tensor x, int64_t R,
                                  int64_t S, int64_t ph, int64_t pw,
                                  c10::optional<torch::Tensor> out,
                                  int64_t strip_rows) {
  TORCH_CHECK(go.is_cuda() && x.is_cuda() && go.get_device() == x.get_device(),
              "tap_bwd_weight_ring: go and x must be on one GPU");
  TORCH_CHECK(go.dim() == 4 && x.dim() == 4 && go.is_contiguous() &&
                  x.is_contiguous(),
              "tap_bwd_weight_ring: go and x must be contiguous 4-d tensors");
  TORCH_CHECK(go.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              "tap_bwd_weight_ring: bf16 only");
  const RingChoice ch = choose_ring(
      x.size(0), x.size(1), go.size(1), x.size(2), x.size(3), R, S, ph, pw,
      ((uintptr_t)x.data_ptr() & 15) == 0, ((uintptr_t)go.data_ptr() & 15) == 0,
      strip_rows);
  const RingGeom& g = ch.g;
  TORCH_CHECK(go.size(0) == g.N && go.size(2) == g.OH && go.size(3) == g.OW,
              "tap_bwd_weight_ring: go is not the gradient of this convolution");
  const int64_t numel = (int64_t)g.K * g.C * R * S;
  torch::Tensor gw;
  if (out.has_value()) {
    gw = *out;
    TORCH_CHECK(gw.is_cuda() && gw.get_device() == go.get_device() &&
                    gw.scalar_type() == torch::kFloat && gw.is_contiguous() &&
                    gw.numel() == numel,
                "tap_bwd_weight_ring: out must be a contiguous fp32 tensor of "
                "K*C*R*S elements on go's device");
  } else {
    gw = torch::zeros({numel}, x.options().dtype(torch::kFloat));
  }
  TORCH_CHECK(ch.blocks < (1LL << 31), "tap_bwd_weight_ring: grid too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(ch.kern, dim3((uint32_t)ch.blocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)go.data_ptr(),
                     (const unsigned short*)x.data_ptr(), gw.data_ptr<float>(),
                     g);
  return gw.view({(int64_t)g.K, (int64_t)g.C, R, S});
}

// ---- weight gradient, pixel-major -------------------------------------------

// The launch of a pixel-major problem: the only place that decides the
// instantiation, the strip length and the grid.
template <int R, int S>
static RingChoice choose_px_rs(RingGeom g, bool xal, bool gal,
                               int64_t strip_rows) {
  using T = PxTile<R, S>;
  constexpr int64_t GRID = 2 * 256;  // one resident block per CU, two rounds
  g.col_bands = (g.OW + T::TW - 1) / T::TW;
  g.k_tiles = (g.K + T::KB - 1) / T::KB;
  g.c_tiles = (g.C + T::CB - 1) / T::CB;
  const int64_t ot = (int64_t)g.k_tiles * g.c_tiles;
  const int64_t bands = (int64_t)g.N * g.col_bands;
  const int64_t row_steps = (g.OH + T::TH - 1) / T::TH;  // steps of one band
  // as choose_ring_rs: `need` strips a band make at least GRID blocks
  // wherever a band has that many steps
  int64_t spb = (strip_rows + T::TH - 1) / T::TH;
  if (strip_rows <= 0) {
    const int64_t need = (GRID + ot * bands - 1) / (ot * bands);
    spb = row_steps / need;
  }
  spb = std::min(std::max<int64_t>(spb, 1), row_steps);
  g.rows = (int)(spb * T::TH);
  g.strips_per_band = (int)((row_steps + spb - 1) / spb);
  const int64_t blocks = ot * bands * g.strips_per_band;
  // the constant shifts are those of pad S / 2: any other pad stages x by
  // elements, at a column offset
  xal = xal && g.pw == T::PWC;
  const RingKern k = xal ? (gal ? tap_bwdw_px_kernel<R, S, true, true>
                                : tap_bwdw_px_kernel<R, S, true, false>)
                         : (gal ? tap_bwdw_px_kernel<R, S, false, true>
                                : tap_bwdw_px_kernel<R, S, false, false>);
  return {k, g, blocks,
          "tap_bwdw_px<" + std::to_string(R) + "x" + std::to_string(S) + "," +
              std::to_string(T::KB) + "x" + std::to_string(T::CB) + ",rows" +
              std::to_string(g.rows) + "," + (xal ? "x16" : "xel") + "," +
              (gal ? "go16" : "goel") + ">"};
}

static RingChoice choose_px(int64_t N, int64_t C, int64_t K, int64_t H,
                            int64_t W, int64_t R, int64_t S, int64_t ph,
                            int64_t pw, bool x_aligned, bool go_aligned,
                            int64_t strip_rows) {
  check_problem(N, C, K, H, W, R, S, ph, pw, "tap_bwd_weight_px");
  RingGeom g;
  g.N = (int)N; g.C = (int)C; g.K = (int)K; g.H = (int)H; g.W = (int)W;
  g.ph = (int)ph; g.pw = (int)pw;
  g.OH = g.H + 2 * g.ph - (int)R + 1;
  g.OW = g.W + 2 * g.pw - (int)S + 1;
  // the kernel addresses one image of x and of go with 32-bit offsets
  TORCH_CHECK(C * H * W < (1LL << 31) && K * g.OH * g.OW < (1LL << 31),
              "tap_bwd_weight_px: problem too large");
  const bool xal = x_aligned && g.W % 8 == 0;
  const bool gal = go_aligned && g.OW % 8 == 0;
  if (R == 1) return choose_px_rs<1, 7>(g, xal, gal, strip_rows);
  if (R == 7) return choose_px_rs<7, 1>(g, xal, gal, strip_rows);
  return choose_px_rs<3, 3>(g, xal, gal, strip_rows);
}

std::string tap_bwdw_px_kernel_name(int64_t N, int64_t C, int64_t K, int64_t H,
                                    int64_t W, int64_t R, int64_t S,
                                    int64_t ph, int64_t pw) {
  return choose_px(N, C, K, H, W, R, S, ph, pw, true, true, 0).label;
}

// tap_bwd_weight's contract on tap_bwdw_px_kernel.
torch::Tensor tap_bwd_weight_px(torch::Tensor go, torch::Tensor x, int64_t R,
                                int64_t S, int64_t ph, int64_t pw,
                                c10::optional<torch::Tensor> out,
                                int64_t strip_rows) {
  TORCH_CHECK(go.is_cuda() && x.is_cuda() && go.get_device() == x.get_device(),
              "tap_bwd_weight_px: go and x must be on one GPU");
  TORCH_CHECK(go.dim() == 4 && x.dim() == 4 && go.is_contiguous() &&
                  x.is_contiguous(),
              "tap_bwd_weight_px: go and x must be contiguous 4-d tensors");
  TORCH_CHECK(go.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              "tap_bwd_weight_px: bf16 only");
  const RingChoice ch = choose_px(
      x.size(0), x.size(1), go.size(1), x.size(2), x.size(3), R, S, ph, pw,
      ((uintptr_t)x.data_ptr() & 15) == 0, ((uintptr_t)go.data_ptr() & 15) == 0,
      strip_rows);
  const RingGeom& g = ch.g;
  TORCH_CHECK(go.size(0) == g.N && go.size(2) == g.OH && go.size(3) == g.OW,
              "tap_bwd_weight_px: go is not the gradient of this convolution");
  const int64_t numel = (int64_t)g.K * g.C * R * S;
  torch::Tensor gw;
  if (out.has_value()) {
    gw = *out;
    TORCH_CHECK(gw.is_cuda() && gw.get_device() == go.get_device() &&
                    gw.scalar_type() == torch::kFloat && gw.is_contiguous() &&
                    gw.numel() == numel,
                "tap_bwd_weight_px: out must be a contiguous fp32 tensor of "
                "K*C*R*S elements on go's device");
  } else {
    gw = torch::zeros({numel}, x.options().dtype(torch::kFloat));
  }
  TORCH_CHECK(ch.blocks < (1LL << 31), "tap_bwd_weight_px: grid too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(ch.kern, dim3((uint32_t)ch.blocks), dim3(256), 0,
                     stream.stream(), (const unsigned short*)go.data_ptr(),
                     (const unsigned short*)x.data_ptr(), gw.data_ptr<float>(),
                     g);
  return gw.view({(int64_t)g.K, (int64_t)g.C, R, S});
}

}  // namespace conv_tap

void register_conv_tap(pybind11::module_& m) {
  m.def("tap_fwd", &conv_tap::tap_fwd, pybind11::arg("x"), pybind11::arg("w"),
        pybind11::arg("bias"), pybind11::arg("ph"), pybind11::arg("pw"),
        pybind11::arg("transposed") = false, pybind11::arg("split") = 0,
        "tap-shift direct stride-1 conv, 1x7 / 7x1 / 3x3 (bf16 NCHW); "
        "transposed: x is the output gradient, w the forward weight, the "
        "result the data gradient; split: 0 one block runs all channels, -1 "
        "the channel chunks are dealt to as many slices as "
        "tap_split_kernel_name says for this device, n > 0 to n slices");
  m.def("tap_kernel_name", &conv_tap::tap_kernel_name,
        "label of the kernel tap_fwd launches for (C, K, H, W, R, S, ph, pw); "
        "no tensor, no HIP call");
  m.def("tap_split_kernel_name", &conv_tap::tap_split_kernel_name,
        "(label, slices) of the launch of tap_fwd(split=-1) for (N, C, K, H, "
        "W, R, S, ph, pw) on a device of `cus` compute units; slices == 1: "
        "tap_kernel_name's kernel; no tensor, no HIP call");
  m.def("tap_fwd_strided", &conv_tap::tap_fwd_strided, pybind11::arg("x"),
        pybind11::arg("w"), pybind11::arg("bias"), pybind11::arg("sh"),
        pybind11::arg("sw"), pybind11::arg("ph"), pybind11::arg("pw"),
        "tap-shift direct strided conv: 1x7 at stride (1, 2), 7x1 at (2, 1), "
        "3x3 at (2, 2) (bf16 NCHW), the input patch staged in phase planes");
  m.def("tap_bwd_data_strided", &conv_tap::tap_bwd_data_strided,
        pybind11::arg("go"), pybind11::arg("w"), pybind11::arg("H"),
        pybind11::arg("W"), pybind11::arg("sh"), pybind11::arg("sw"),
        pybind11::arg("ph"), pybind11::arg("pw"),
        "data gradient [N, C, H, W] of the convolution tap_fwd_strided runs, "
        "by phase decomposition of go (no zero-stuffing); w is the forward "
        "weight");
  m.def("tap_strided_kernel_name", &conv_tap::tap_strided_kernel_name,
        pybind11::arg("C"), pybind11::arg("K"), pybind11::arg("H"),
        pybind11::arg("W"), pybind11::arg("R"), pybind11::arg("S"),
        pybind11::arg("sh"), pybind11::arg("sw"), pybind11::arg("ph"),
        pybind11::arg("pw"), pybind11::arg("transposed") = false,
        "label of the kernel tap_fwd_strided or (transposed: C the reduction "
        "dim, K the output channels of the launch) tap_bwd_data_strided "
        "launches; H x W is the forward's input; no tensor, no HIP call");
  m.def("tap_bwd_weight", &conv_tap::tap_bwd_weight, pybind11::arg("go"),
        pybind11::arg("x"), pybind11::arg("R"), pybind11::arg("S"),
        pybind11::arg("ph"), pybind11::arg("pw"),
        pybind11::arg("out") = pybind11::none(),
        pybind11::arg("tiles_per_block") = 0,
        "tap-shift MFMA weight gradient of a stride-1 1x7 / 7x1 / 3x3 conv "
        "(bf16 NCHW in, fp32 [K, C, R, S] out); adds into `out` when given; "
        "tiles_per_block > 0 overrides the chooser's run length");
  m.def("tap_bwdw_kernel_name", &conv_tap::tap_bwdw_kernel_name,
        "label of the kernel tap_bwd_weight launches for (N, C, K, H, W, R, S, "
        "ph, pw); no tensor, no HIP call");
  m.def("tap_bwd_weight_ring", &conv_tap::tap_bwd_weight_ring,
        pybind11::arg("go"), pybind11::arg("x"), pybind11::arg("R"),
        pybind11::arg("S"), pybind11::arg("ph"), pybind11::arg("pw"),
        pybind11::arg("out") = pybind11::none(),
        pybind11::arg("strip_rows") = 0,
        "tap_bwd_weight on the rolling-window kernel: a block walks a strip "
        "of output rows and stages only the new rows of a step; strip_rows > 0 "
        "overrides the chooser's strip length");
  m.def("tap_bwdw_ring_kernel_name", &conv_tap::tap_bwdw_ring_kernel_name,
        "label of the kernel tap_bwd_weight_ring launches for (N, C, K, H, W, "
        "R, S, ph, pw); no tensor, no HIP call");
  m.def("tap_bwd_weight_px", &conv_tap::tap_bwd_weight_px, pybind11::arg("go"),
        pybind11::arg("x"), pybind11::arg("R"), pybind11::arg("S"),
        pybind11::arg("ph"), pybind11::arg("pw"),
        pybind11::arg("out") = pybind11::none(),
        pybind11::arg("strip_rows") = 0,
        "tap_bwd_weight on the pixel-major kernel: go and x staged as they "
        "lie in memory, column taps shifted in registers; strip_rows > 0 "
        "overrides the chooser's strip length");
  m.def("tap_bwdw_px_kernel_name", &conv_tap::tap_bwdw_px_kernel_name,
        "label of the kernel tap_bwd_weight_px launches for (N, C, K, H, W, "
        "R, S, ph, pw); no tensor, no HIP call");
}
