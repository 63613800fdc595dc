// Persistent weight-stationary pointwise GEMM (bf16 MFMA, fp32 accumulate).
//
//   D[b][t][n] = sum_k A[b][t][k] * W[n][k]      for the FULL n range of one layer
//
// Why: with 128x128 tiles the 1x1 convolutions of the TCN block were bound by
// L2 -> LDS traffic (every tile re-streams its weights: ~12 TB/s measured) instead of
// HBM. Here one workgroup (8 waves) per CU keeps the whole weight matrix of the layer
// in REGISTERS -- wave w owns NSL output channels for all Kp inputs (NSL*Kp <= 16384
// -> <= 128 VGPRs) -- and streams 32-frame A tiles through a double-buffered LDS
// ring: one barrier per tile, A prefetched one tile ahead into registers. Each wave
// stages its accumulator sub-tile in a private LDS region and runs the row-wise
// epilogue on it (no second barrier).
//
// The loop body is branch-free around memory operations: every global access is a
// buffer_load / buffer_store through a per-item descriptor, so frames past the end of
// an item (and the padding tile of an odd tile count) read zeros and drop their stores
// in hardware. That keeps the compiler's s_waitcnt counted (vmcnt(N), never a drain)
// and the prefetches in flight across the barrier.
//
// Instances: 128->512 (pw1_fwd, bottleneck_dgrad, last pw2_dgrad), 512->256
// (pw2_fwd), 256->512 (pw2_dgrad). Anything else goes through gemm_rows_kernel.
#pragma once
#include "gemm_rows.cuh"
#include "tcn_kernels.cuh"
#include "gfx950.cuh"

namespace brv {


template <int KP, int NSL, int WM, int NW = 8>
struct GemmWsCfg {
  static constexpr int NTHR = 64*NW;           // threads per workgroup
  static constexpr int WN = NW/WM;
  static constexpr int NP = WN*NSL;            // full output width
  static constexpr int BMW = 32*WM;            // frames per workgroup tile
  static constexpr int NF = NSL/32;            // 32x32 MFMA tiles per wave
  static constexpr int KS = KP/16;             // MFMA k-steps
  static constexpr int LDA = KP + 8;           // padded LDS row (conflict-free b128)
  static constexpr int LDW = NSL + 4;          // fp32 staging row of one wave
  static constexpr int ACH = BMW*KP/8/NTHR;    // 16-byte A chunks per thread
  static constexpr int kA = 2*BMW*LDA*2;
  static constexpr int kC = NW*32*LDW*4;
  static constexpr int kSmem = kA + kC + 2*KP*4;
  // The dispatcher does not balance workgroups over CUs by itself: with room for more,
  // it stacks several of these persistent workgroups on one CU and leaves others idle
  // (measured: median workgroup 23 us, slowest 36 us). Claiming more than 1/2 (8 waves)
  // or 1/3 (4 waves) of the 160 KB LDS caps residency at exactly the 1 or 2 workgroups
  // per CU the grid is sized for, which forces an even spread.
  static constexpr int kWgPerCu = NW == 8 ? 1 : 2;
  static constexpr int kSmemMin = NW == 8 ? 84*1024 : 56*1024;
  static constexpr int kSmemAlloc = kSmem > kSmemMin ? kSmem : kSmemMin;
  static_assert(kSmemAlloc*kWgPerCu <= 160*1024, "LDS budget");
};

// AT: 0 = A used as stored, 1 = PReLU + gLN affine applied while staging,
//     2 = lazy residual: A = x + rstd*u + c built while staging and written back (the block input
//         the previous block's fused [res | skip] product left unfinished, see AT == 3),
//     3 = fused depthwise stage: A = PReLU_2(z2) with z2 = dconv(gLN_1(PReLU_1(z1))) + bias
//         computed while staging from three dilated taps of z1; z2 is stored for the backward
//         pass, the statistics of PReLU_2(z2) are accumulated, and the second norm is NOT
//         applied: W.gLN(p) = rstd (W gamma) p + (W beta - mean rstd W gamma 1) is linear in p,
//         so the product runs on p with gamma-folded weights and the per-item scale / offset
//         are applied by the consumers (AT == 2 and skip_combine_kernel).
// CAT: A is the concatenation [p0 | p1] along k (split at a.K0).
template <int KP, int NSL, int WM, int EM, int AT, bool CAT, int NW = 8>
__global__ __launch_bounds__(64*NW) void gemm_ws_kernel(const GemmRowsParams p) {
  using C = GemmWsCfg<KP, NSL, WM, NW>;
  static_assert(C::ACH >= 1, "tile too small for the workgroup");
  __shared__ __attribute__((aligned(16))) unsigned char smem[C::kSmemAlloc];
  bf16_t* As = reinterpret_cast<bf16_t*>(smem);
  float* Cw_all = reinterpret_cast<float*>(smem + C::kA);
  float* scs = reinterpret_cast<float*>(smem + C::kA + C::kC);      // [KP] scale
  float* shs = scs + KP;                                             // [KP] shift
  // AT == 3: per-channel stencil tables [10][KP]: tap k < 3: wa_k (z), 3 + k: wb_k (|z|),
  // 6 + k: constant term of tap k, 9: bias
  __shared__ __attribute__((aligned(16))) float tabs[AT == 3 ? 10*KP : 4];
  static_assert(AT != 3 || C::kSmemAlloc + 10*KP*4 <= 160*1024, "LDS budget (fused stage)");
  constexpr int NA = AT == 2 ? 2 : (AT == 3 ? 3 : 1);                // raw chunks per staged chunk

#ifdef BRV_DIAG
  const long long t_entry = stamp_cycles();
  const long long r_entry = stamp_realtime();
#endif
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / C::WN, wn = wid % C::WN;
  const int fr = lane & 31, fh = lane >> 5;
  const int T = p.T;
  const ASpec& a = p.a;
  const EpiSpec& e = p.e;
  float* Cw = Cw_all + wid*32*C::LDW;

  // ---- weights of this wave's channel slice -> registers ------------------------
  bf16x8 wf[C::NF][C::KS];
  {
    // blockIdx.y selects a group of NP output channels when the layer is wider than
    // what one workgroup keeps in registers
    // Wp: the same weights re-packed by brv_ctn_prepare in fragment order (slice, f, s,
    // lane, 8 values), so that every load instruction reads 1 KiB contiguous; the plain
    // [N][K] layout makes each instruction touch 32 rows x 32 B (4x the L2 requests in the
    // prologue every workgroup runs at the same time: pw2_fwd -7 %)
    const bool packed = p.Wp != nullptr && p.wp_nsl == NSL;
    const bf16_t* wbase = (packed ? p.Wp : p.W) + (long long)(blockIdx.y*C::NP + wn*NSL)*KP;
#pragma unroll
    for (int f = 0; f < C::NF; ++f)
#pragma unroll
      for (int s = 0; s < C::KS; ++s)
        wf[f][s] = *reinterpret_cast<const bf16x8*>(
            packed ? wbase + ((long long)(f*C::KS + s)*64 + lane)*8
                   : wbase + (long long)(32*f + fr)*KP + 16*s + 8*fh);
  }

  // ---- tile schedule: contiguous range per workgroup ------------------------------
  const int tpi = ceil_div(T, C::BMW);                 // tiles per item
  const int total = tpi*p.batch;
  const int per = ceil_div(total, (int)gridDim.x);
#ifdef BRV_DIAG
  if ((p.dbg & 256) && gridDim.y > 1 && blockIdx.y == 0) return;   // only the second column group runs
  if ((p.dbg & 32) && blockIdx.x < gridDim.x/2) return;       // only the later-dispatched half runs
  if ((p.dbg & 128) && blockIdx.x >= gridDim.x/2) return;     // only the first half runs
  const int t_begin = ((p.dbg & 16) ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x)*per;
#else
  const int t_begin = blockIdx.x*per;
#endif
  const int t_end = min(total, t_begin + per);
  const int t_items = tpi*C::BMW;                      // frame count rounded up to tiles

  // ---- A staging geometry (fixed k chunk per thread) -------------------------------
  constexpr int CPR = KP/8;                            // chunks per frame
  constexpr int RSTEP = C::NTHR/CPR;
  const int kc = tid % CPR;
  const int arow0 = tid / CPR;                         // + RSTEP*ci
  const int kbase = kc*8;
  const float slope = ((AT == 1 || AT == 3) && a.slope) ? *a.slope : 1.f;
  const float slope2 = (AT == 3 && a.slope2) ? *a.slope2 : 1.f;
  const bool first = !CAT || kbase < a.K0;
  const unsigned int akoff = (unsigned int)((first ? kbase : kbase - a.K0)*2);

#ifdef BRV_DIAG
  const int dbg = p.dbg;                               // ablation flags (tools/ablate.py)
#else
  constexpr int dbg = 0;
#endif
  // (b, t0) = item and first frame of the tile; `valid` false -> every lane reads zeros
  auto load_tile = [&](int b, int t0, bool valid, uint4 (&araw)[C::ACH*NA]) {
    if (dbg & 8) valid = false;
    const __amdgpu_buffer_rsrc_t r0 = make_rsrc(
        reinterpret_cast<const bf16_t*>(a.p0) + (long long)b*a.bs0,
        valid ? (long long)T*a.ld0*2 : 0);
#pragma unroll
    for (int ci = 0; ci < C::ACH; ++ci) {
      const unsigned int t = (unsigned int)(t0 + arow0 + RSTEP*ci);
      if (AT == 2) {
        const __amdgpu_buffer_rsrc_t r1 = make_rsrc(
            reinterpret_cast<const bf16_t*>(a.p1) + (long long)b*a.bs1,
            valid ? (long long)T*a.ld1*2 : 0);
        araw[2*ci] = buf_load16(r0, t*(unsigned int)(a.ld0*2) + akoff);
        araw[2*ci + 1] = buf_load16(r1, t*(unsigned int)(a.ld1*2) + akoff);
      } else if (AT == 3) {
        // taps outside [0, T) wrap to offsets beyond the descriptor: zeros
#pragma unroll
        for (int k = 0; k < 3; ++k)
          araw[3*ci + k] = buf_load16(r0, (t + (unsigned int)(k*a.dil - a.left))*(unsigned int)(a.ld0*2) + akoff);
      } else if (!CAT) {
        araw[ci] = buf_load16(r0, t*(unsigned int)(a.ld0*2) + akoff);
      } else {
        const __amdgpu_buffer_rsrc_t r1 = make_rsrc(
            reinterpret_cast<const bf16_t*>(a.p1) + (long long)b*a.bs1,
            valid ? (long long)T*a.ld1*2 : 0);
        const uint4 x0 = buf_load16(r0, first ? t*(unsigned int)(a.ld0*2) + akoff : kOob);
        const uint4 x1 = buf_load16(r1, first ? kOob : t*(unsigned int)(a.ld1*2) + akoff);
        araw[ci] = make_uint4(x0.x | x1.x, x0.y | x1.y, x0.z | x1.z, x0.w | x1.w);
      }
    }
  };
  double a_sum = 0.0, a_sq = 0.0;          // AT == 3: statistics of PReLU_2(z2), current item
  int a_item = -1;
  auto flush_astats = [&]() {
    if (AT != 3 || a_item < 0) return;
    const double s0 = wave_sum(a_sum), s1 = wave_sum(a_sq);
    if (lane == 0) {
      atomic_add_f64(a.stats2_out + stat_sum(a_item), s0);
      atomic_add_f64(a.stats2_out + stat_sq(a_item), s1);
    }
    a_sum = 0.0; a_sq = 0.0;
  };
  auto store_tile = [&](int b, int t0, int buf, const uint4 (&araw)[C::ACH*NA]) {
    bf16_t* dst = As + buf*C::BMW*C::LDA;
    if (AT == 2) {
      // x_next = x + rstd*u + c (c, rstd: per-item table built by update_affine)
      const __amdgpu_buffer_rsrc_t rx = make_rsrc(
          reinterpret_cast<bf16_t*>(a.xout) + (long long)b*a.bs0, (long long)T*a.ld0*2);
      const float rl = shs[0];
      float cl[8];
      {
        const float4 c0 = *reinterpret_cast<const float4*>(scs + kbase);
        const float4 c1 = *reinterpret_cast<const float4*>(scs + kbase + 4);
        cl[0] = c0.x; cl[1] = c0.y; cl[2] = c0.z; cl[3] = c0.w;
        cl[4] = c1.x; cl[5] = c1.y; cl[6] = c1.z; cl[7] = c1.w;
      }
#pragma unroll
      for (int ci = 0; ci < C::ACH; ++ci) {
        const int row = arow0 + RSTEP*ci;
        float f[8], u[8];
        unpack8(araw[2*ci], f); unpack8(araw[2*ci + 1], u);
        const float live = (t0 + row < T) ? 1.f : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = live*(f[j] + __builtin_fmaf(rl, u[j], cl[j]));
        const uint4 q = pack8(f);
        buf_store16(rx, (unsigned int)(t0 + row)*(unsigned int)(a.ld0*2) + akoff, q);   // t >= T: dropped
        *reinterpret_cast<uint4*>(dst + row*C::LDA + kbase) = q;
      }
      return;
    }
    if (AT == 3) {
      const __amdgpu_buffer_rsrc_t rz = make_rsrc(
          reinterpret_cast<bf16_t*>(a.z2out) + (long long)b*a.bs0, (long long)T*a.ld0*2);
      if (b != a_item) { flush_astats(); a_item = b; }
      auto ld8 = [&](int which, float (&v)[8]) {
        const float4 x0 = *reinterpret_cast<const float4*>(tabs + which*KP + kbase);
        const float4 x1 = *reinterpret_cast<const float4*>(tabs + which*KP + kbase + 4);
        v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w;
        v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
      };
      const float d1 = 0.5f*(1.f + slope2), d2 = 0.5f*(1.f - slope2);
      float ts = 0.f, tq = 0.f;
      // rows in groups of RG; the per-channel tables are re-read from LDS per group. Measured:
      // RG = 2 (fewer live registers) costs 28 us per launch in LDS reads, so all rows go at once
      constexpr int RG = C::ACH;
#pragma unroll
      for (int c0i = 0; c0i < C::ACH; c0i += RG) {
        float acc[RG][8];
        // constant terms: bias + the taps that fall inside the item (wave-uniform per row)
        {
          float bs[8];
          ld8(9, bs);
#pragma unroll
          for (int g = 0; g < RG; ++g)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[g][j] = bs[j];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float wa[8], wb[8], wc[8];
          ld8(k, wa); ld8(3 + k, wb); ld8(6 + k, wc);
#pragma unroll
          for (int g = 0; g < RG; ++g) {
            const int ci = c0i + g;
            const int ti = t0 + arow0 + RSTEP*ci + k*a.dil - a.left;
            const float in = (ti >= 0 && ti < T) ? 1.f : 0.f;
            float f[8];
            unpack8(araw[3*ci + k], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              acc[g][j] = __builtin_fmaf(in, wc[j], acc[g][j]);
              acc[g][j] = __builtin_fmaf(wa[j], f[j], acc[g][j]);
              acc[g][j] = __builtin_fmaf(wb[j], __builtin_fabsf(f[j]), acc[g][j]);
            }
          }
        }
#pragma unroll
        for (int g = 0; g < RG; ++g) {
          const int row = arow0 + RSTEP*(c0i + g);
          const uint4 q = pack8(acc[g]);
          buf_store16(rz, (unsigned int)(t0 + row)*(unsigned int)(a.ld0*2) + akoff, q);   // t >= T: dropped
          float r[8], pv[8];
          unpack8(q, r);
          const float live = (t0 + row < T) ? 1.f : 0.f;
          float fs = 0.f, fq = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            pv[j] = live*__builtin_fmaf(d2, __builtin_fabsf(r[j]), d1*r[j]);
            fs += pv[j]; fq = __builtin_fmaf(pv[j], pv[j], fq);
          }
          ts += fs; tq += fq;
          *reinterpret_cast<uint4*>(dst + row*C::LDA + kbase) = pack8(pv);
        }
      }
      a_sum += (double)ts; a_sq += (double)tq;
      return;
    }
    float sc[8], sh[8];
    if (AT == 1) {
      const float4 s0 = *reinterpret_cast<const float4*>(scs + kbase);
      const float4 s1 = *reinterpret_cast<const float4*>(scs + kbase + 4);
      const float4 h0 = *reinterpret_cast<const float4*>(shs + kbase);
      const float4 h1 = *reinterpret_cast<const float4*>(shs + kbase + 4);
      sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w;
      sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w;
      sh[0] = h0.x; sh[1] = h0.y; sh[2] = h0.z; sh[3] = h0.w;
      sh[4] = h1.x; sh[5] = h1.y; sh[6] = h1.z; sh[7] = h1.w;
    }
#pragma unroll
    for (int ci = 0; ci < C::ACH; ++ci) {
      const int row = arow0 + RSTEP*ci;
      uint4 q = araw[ci];
      if (AT == 1) {
        float f[8];
        unpack8(q, f);
        // rows past the end were read as zeros, but the affine shift would make them
        // non-zero: scale the result by the row validity
        const float live = (t0 + row < T) ? 1.f : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = live*(prelu(f[j], slope)*sc[j] + sh[j]);
        q = pack8(f);
      }
      *reinterpret_cast<uint4*>(dst + row*C::LDA + kbase) = q;
    }
  };
  // per-item gLN scale/shift table in LDS (rebuilt when the item changes: rare)
  int cur_item = -1;
  auto update_affine = [&](int b) {
    if (AT == 0 || b == cur_item) return;
    __syncthreads();
    if (AT == 1 && tid < KP) {
      const NormStat ns = norm_stat(a.stats, b, a.inv_n, a.eps);
      const float g = tid < a.C ? a.gamma[tid] : 0.f;
      const float be = tid < a.C ? a.beta[tid] : 0.f;
      scs[tid] = ns.rstd*g;
      shs[tid] = be - ns.mean*ns.rstd*g;
    }
    if (AT == 2 && tid < KP) {
      const NormStat ns = norm_stat(a.stats, b, a.inv_n, a.eps);
      scs[tid] = a.lazy_v0[tid] - ns.mean*ns.rstd*a.lazy_v1[tid];
      if (tid == 0) shs[0] = ns.rstd;
    }
    if (AT == 3) {
      const NormStat ns = norm_stat(a.stats, b, a.inv_n, a.eps);
      const float c1 = 0.5f*(1.f + slope), c2 = 0.5f*(1.f - slope);
      for (int c = tid; c < KP; c += C::NTHR) {
        const bool ok = c < a.C;
        const float g = ok ? a.gamma[c] : 0.f, be = ok ? a.beta[c] : 0.f;
        const float scv = ns.rstd*g, shv = be - ns.mean*ns.rstd*g;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float w = ok ? a.taps[c*3 + k] : 0.f;
          tabs[k*KP + c] = w*c1*scv; tabs[(3 + k)*KP + c] = w*c2*scv; tabs[(6 + k)*KP + c] = w*shv;
        }
        tabs[9*KP + c] = ok ? a.dbias[c] : 0.f;
      }
    }
    __syncthreads();
    cur_item = b;
  };

  // ---- epilogue state (wave-private) -------------------------------------------------
  // The MFMA runs as D^T = W * A^T: a lane holds ONE frame (lane & 31) and, per 32-channel
  // chunk, four runs of 4 consecutive channels -> the accumulators go to the staging
  // tile as 16-byte LDS writes and come back as rows of 8 channels per lane.
  constexpr int CH = NSL/8;                            // 8-column chunks per staged row
  constexpr int RPP = 64/CH;                           // rows per pass
  constexpr int NPASS = 32/RPP;
  const int ech = lane % CH, erow0 = lane / CH;
  const int ncol = blockIdx.y*C::NP + wn*NSL + ech*8;  // global output column of the chunk
  // bias: folded into the accumulator initialisation (register i of chunk f is channel
  // 32f + (i & 3) + 8(i >> 2) + 4(lane >> 5) of this wave's slice)
  constexpr bool kBias = (EM == E_STORE || EM == E_RES_SKIP) && AT != 3;   // the fused stage has no bias
  float bias_r[kBias ? C::NF : 1][16];
  if (kBias) {
#pragma unroll
    for (int f = 0; f < C::NF; ++f)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int n = blockIdx.y*C::NP + wn*NSL + 32*f + (i & 3) + 8*(i >> 2) + 4*fh;
        const bool second = EM == E_RES_SKIP && n >= e.Nsplit;
        const float* bp = second ? e.bias2 : e.bias;
        const int idx = second ? n - e.Nsplit : n;
        int lim = second ? e.N2 : e.N;
        // unconditional (clamped) load + select: the 16*NF loads stay in flight together;
        // a missing bias reads the weights instead and is masked to zero
        if (bp == nullptr) { bp = reinterpret_cast<const float*>(p.W); lim = 0; }
        const float x = bp[idx < lim ? idx : (lim > 0 ? lim - 1 : 0)];
        bias_r[f][i] = idx < lim ? x : 0.f;
      }
  }
  float gam[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) gam[j] = 0.f;
  const bool is_res = EM == E_RES_SKIP && ncol < e.Nsplit;
  if (EM == E_GLN_BWD) load8_masked(e.gamma, ncol, e.N, gam);
  const float eslope = (EM == E_GLN_BWD && e.src_slope) ? *e.src_slope
                     : (EM == E_STORE && e.stats_slope ? *e.stats_slope : 1.f);
  // prelu(r) = c1*r + c2*|r|: two VALU ops (|r| is a source modifier), no compare/select
  const float c1 = 0.5f*(1.f + eslope), c2 = 0.5f*(1.f - eslope);
  const bool want_stats = EM == E_STORE && e.stats_out != nullptr;
  const float skip_keep = (EM == E_RES_SKIP && !e.skip_init) ? 1.f : 0.f;
  double st_sum = 0.0, st_sq = 0.0;
  int st_item = -1;
  f32x2 colA[4], colB[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { colA[j] = f32x2{0.f, 0.f}; colB[j] = f32x2{0.f, 0.f}; }

  auto flush_stats = [&]() {
    if (st_item < 0) return;
    if (want_stats || EM == E_GLN_BWD) {
      const double s0 = wave_sum(st_sum), s1 = wave_sum(st_sq);
      double* dst = (EM == E_STORE) ? e.stats_out : e.sums_out;
      if (lane == 0 && !(dbg & 1024)) {
        atomic_add_f64(dst + stat_sum(st_item), s0);
        atomic_add_f64(dst + stat_sq(st_item), s1);
      }
    }
    st_sum = 0.0; st_sq = 0.0;
  };

#ifdef BRV_DIAG
  long long cyc_mfma = 0, cyc_epi = 0, cyc_stage = 0, cyc_total0 = 0;
#define BRV_STAMP(expr) do { if (dbg & 64) { expr; } } while (0)
#else
#define BRV_STAMP(expr) do { } while (0)
#endif
  // compute + epilogue of one tile (item b, first frame t0w for this wave) whose A
  // operand sits in LDS buffer `buf`
  auto process_tile = [&](int b, int t0, int buf) {
#ifdef BRV_DIAG
    long long ts0 = 0, ts1 = 0;
#endif
    BRV_STAMP(ts0 = stamp_cycles());
    const long long recs = (dbg & 1) ? 0 : 1;
    // per-item descriptors: frames >= T fall outside and are dropped / read as zero
    const __amdgpu_buffer_rsrc_t rout = make_rsrc(
        reinterpret_cast<const bf16_t*>(e.out) + (long long)b*T*e.ldo, recs*T*e.ldo*2);
    __amdgpu_buffer_rsrc_t rc0 = rout, rc1 = rout;
    if (EM == E_RES_SKIP) {
      rc0 = make_rsrc(e.res_in + (long long)b*T*e.ld_res, recs*T*e.ld_res*2);
      rc1 = make_rsrc(e.skip + (long long)b*T*e.ld_skip, recs*T*e.ld_skip*4);
    } else if (EM == E_GLN_BWD) {
      rc0 = make_rsrc(e.src + (long long)b*T*e.ld_src, recs*T*e.ld_src*2);
    } else if (EM == E_ADD) {
      rc0 = make_rsrc(e.add_in + (long long)b*T*e.ld_add, e.add_in ? recs*T*e.ld_add*2 : 0);
    }
    // companion tensors of the row-wise epilogue: loads issued before the MFMAs
    uint4 comp0[NPASS], comp1[(EM == E_RES_SKIP) ? NPASS : 1];
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
      const unsigned int t = (unsigned int)(t0 + erow0 + RPP*pass);
      if (EM == E_RES_SKIP) {
        const unsigned int so = (t*(unsigned int)e.ld_skip + (unsigned int)(ncol - e.Nsplit))*4u;
        comp0[pass] = is_res
            ? buf_load16(rc0, (t*(unsigned int)e.ld_res + (unsigned int)ncol)*2u)
            : buf_load16(rc1, so);
        comp1[pass] = buf_load16(rc1, is_res ? kOob : so + 16u);
      } else if (EM == E_GLN_BWD) {
        comp0[pass] = buf_load16(rc0, (t*(unsigned int)e.ld_src + (unsigned int)ncol)*2u);
      } else if (EM == E_ADD) {
        comp0[pass] = buf_load16(rc0, (t*(unsigned int)e.ld_add + (unsigned int)ncol)*2u);
      } else {
        comp0[pass] = make_uint4(0, 0, 0, 0);
      }
    }

    f32x16 acc[C::NF];
#pragma unroll
    for (int f = 0; f < C::NF; ++f)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[f][i] = kBias ? bias_r[kBias ? f : 0][i] : 0.f;
    const bf16_t* abuf = As + buf*C::BMW*C::LDA + (32*wm + fr)*C::LDA + 8*fh;
    if (!(dbg & 4))
#pragma unroll
    for (int s = 0; s < C::KS; ++s) {
      const bf16x8 af = *reinterpret_cast<const bf16x8*>(abuf + 16*s);
#pragma unroll
      for (int f = 0; f < C::NF; ++f)
        acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[f][s], af, acc[f], 0, 0, 0);
    }
    if (dbg & 2) {
      if (acc[0][0] == 123.456f) Cw[0] = acc[0][1];     // keep the MFMAs alive
      return;
    }
    // accumulators -> this wave's private fp32 staging tile [32 frames][NSL]
#pragma unroll
    for (int f = 0; f < C::NF; ++f)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(Cw + fr*C::LDW + 32*f + 8*g + 4*fh) =
            make_float4(acc[f][4*g], acc[f][4*g + 1], acc[f][4*g + 2], acc[f][4*g + 3]);

    BRV_STAMP(ts1 = stamp_cycles(); cyc_mfma += ts1 - ts0);
    if (b != st_item) { flush_stats(); st_item = b; }
    float mrs = 0.f;                                    // -mean*rstd
    float rstd = 1.f;
    if (EM == E_GLN_BWD) {
      const NormStat es = norm_stat(e.src_stats, b, e.inv_n, e.eps);
      rstd = es.rstd; mrs = -es.mean*es.rstd;
    }

    float tile_s = 0.f, tile_q = 0.f;
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
      const int row = erow0 + RPP*pass;
      const unsigned int t = (unsigned int)(t0 + row);
      const float4 lo = *reinterpret_cast<const float4*>(Cw + row*C::LDW + ech*8);
      const float4 hi = *reinterpret_cast<const float4*>(Cw + row*C::LDW + ech*8 + 4);
      f32x2 v[4] = {f32x2{lo.x, lo.y}, f32x2{lo.z, lo.w}, f32x2{hi.x, hi.y}, f32x2{hi.z, hi.w}};
      const unsigned int ooff = (t*(unsigned int)e.ldo + (unsigned int)ncol)*2u;
      if (EM == E_STORE) {
        const uint4 q = pack8v(v);
        buf_store16(rout, ooff, q);
        if (want_stats) {                               // wave-uniform, VALU only inside
          float r[8]; unpack8(q, r);
          f32x2 ls = {0.f, 0.f}, lq = {0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            f32x2 pv;
            pv.x = __builtin_fmaf(c2, __builtin_fabsf(r[2*j]), c1*r[2*j]);
            pv.y = __builtin_fmaf(c2, __builtin_fabsf(r[2*j + 1]), c1*r[2*j + 1]);
            ls += pv; lq += pv*pv;
          }
          // frames past the end of the item hold the bias, not zero: mask the row
          const float rm = (int)t < T ? 1.f : 0.f;
          tile_s = __builtin_fmaf(rm, ls.x + ls.y, tile_s);
          tile_q = __builtin_fmaf(rm, lq.x + lq.y, tile_q);
        }
      } else if (EM == E_RES_SKIP) {
        if (is_res) {                               // wave-uniform
          float r[8];
          unpack8(comp0[pass], r);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += f32x2{r[2*j], r[2*j + 1]};
          buf_store16(rout, ooff, pack8v(v));
        } else {
          const uint4 c0 = comp0[pass];
          const uint4 c1q = comp1[(EM == E_RES_SKIP) ? pass : 0];
          // first block: the skip buffer is uninitialised memory -- a SELECT, not a product with zero
          // (0 x NaN = NaN: whole outputs were NaN when the workspace reused freed memory holding NaNs)
          if (skip_keep != 0.f) {
            v[0] += f32x2{__uint_as_float(c0.x), __uint_as_float(c0.y)};
            v[1] += f32x2{__uint_as_float(c0.z), __uint_as_float(c0.w)};
            v[2] += f32x2{__uint_as_float(c1q.x), __uint_as_float(c1q.y)};
            v[3] += f32x2{__uint_as_float(c1q.z), __uint_as_float(c1q.w)};
          }
          const unsigned int so = (t*(unsigned int)e.ld_skip + (unsigned int)(ncol - e.Nsplit))*4u;
          buf_store16(rc1, so, make_uint4(__float_as_uint(v[0].x), __float_as_uint(v[0].y),
                                          __float_as_uint(v[1].x), __float_as_uint(v[1].y)));
          buf_store16(rc1, so + 16u, make_uint4(__float_as_uint(v[2].x), __float_as_uint(v[2].y),
                                                __float_as_uint(v[3].x), __float_as_uint(v[3].y)));
        }
      } else if (EM == E_GLN_BWD) {
        float s[8];
        unpack8(comp0[pass], s);
        // A rows past the end are zero, so v == 0 there: no row mask needed
        f32x2 l1 = {0.f, 0.f}, l2 = {0.f, 0.f}, o[4];
        const f32x2 rs2 = {rstd, rstd}, mrs2 = {mrs, mrs};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f32x2 pv;
          pv.x = __builtin_fmaf(c2, __builtin_fabsf(s[2*j]), c1*s[2*j]);
          pv.y = __builtin_fmaf(c2, __builtin_fabsf(s[2*j + 1]), c1*s[2*j + 1]);
          const f32x2 xh = pv*rs2 + mrs2;
          const f32x2 ev = f32x2{gam[2*j], gam[2*j + 1]}*v[j];
          o[j] = ev;
          l1 += ev; l2 += ev*xh;
          colA[j] += v[j]*xh; colB[j] += v[j];
        }
        tile_s += l1.x + l1.y; tile_q += l2.x + l2.y;
        buf_store16(rout, ooff, pack8v(o));
      } else if (EM == E_ADD) {
        float r[8];
        unpack8(comp0[pass], r);                    // zeros when add_in is null
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += f32x2{r[2*j], r[2*j + 1]};
        buf_store16(rout, ooff, pack8v(v));
      }
    }
    st_sum += (double)tile_s; st_sq += (double)tile_q;
    BRV_STAMP(cyc_epi += stamp_cycles() - ts1);
  };

  // ---- main loop: A prefetched one tile ahead behind counted waits; (b, t0) of the
  // current and the next tile advance incrementally (no integer division per tile) ------
#ifndef GW_AHEAD
#define GW_AHEAD 1       // A tiles requested ahead of the one being multiplied (2: VERDICT r4 item 1b, measured in DESIGN 5m)
#endif
  uint4 araw[C::ACH*NA];
#if GW_AHEAD == 2
  uint4 araw2[C::ACH*NA];
#endif
  if (t_begin < t_end) {
    int b_cur = t_begin / tpi, t_cur = (t_begin % tpi)*C::BMW;
    load_tile(b_cur, t_cur, true, araw);
#if GW_AHEAD == 2
    int b_n1 = b_cur, t_n1 = t_cur + C::BMW;
    if (t_n1 >= t_items) { t_n1 = 0; ++b_n1; }
    load_tile(t_begin + 1 < t_end ? b_n1 : b_cur, t_n1, t_begin + 1 < t_end, araw2);
#endif
    if (EM == E_STORE) {
      // vmcnt bookkeeping: the compiler merges the wait state of the loop entry with the
      // back edge; the same number of younger VMEM ops on both paths keeps the wait on
      // the A prefetch counted (vmcnt(NPASS)) instead of a full drain of the stores
      const __amdgpu_buffer_rsrc_t rnull = make_rsrc(e.out, 0);
#pragma unroll
      for (int pass = 0; pass < NPASS; ++pass) buf_store16(rnull, kOob - 32u*pass, make_uint4(pass, 0, 0, 0));
    }
    int buf = 0;
    BRV_STAMP(cyc_total0 = stamp_cycles());
#if GW_AHEAD == 2
    // two tiles in flight: the loop walks pairs of tiles so that the two register sets alternate statically
    auto one = [&](int tile, uint4 (&ar)[C::ACH*NA]) {
      update_affine(b_cur);
      store_tile(b_cur, t_cur, buf, ar);
      __syncthreads();
      int b_nxt = b_cur, t_nxt = t_cur + C::BMW;
      if (t_nxt >= t_items) { t_nxt = 0; ++b_nxt; }
      int b_n2 = b_nxt, t_n2 = t_nxt + C::BMW;
      if (t_n2 >= t_items) { t_n2 = 0; ++b_n2; }
      const bool more2 = tile + 2 < t_end;
      load_tile(more2 ? b_n2 : b_cur, t_n2, more2, ar);
      process_tile(b_cur, t_cur + 32*wm, buf);
      b_cur = b_nxt; t_cur = t_nxt; buf ^= 1;
    };
#pragma unroll 1
    for (int tile = t_begin; tile < t_end; tile += 2) {
      one(tile, araw);
      if (tile + 1 < t_end) one(tile + 1, araw2);
    }
#else
#pragma unroll 1
    for (int tile = t_begin; tile < t_end; ++tile, buf ^= 1) {
#ifdef BRV_DIAG
      long long tq = 0;
#endif
      BRV_STAMP(tq = stamp_cycles());
      update_affine(b_cur);
      store_tile(b_cur, t_cur, buf, araw);
      __syncthreads();
      int b_nxt = b_cur, t_nxt = t_cur + C::BMW;
      if (t_nxt >= t_items) { t_nxt = 0; ++b_nxt; }
      const bool more = tile + 1 < t_end;
      load_tile(more ? b_nxt : b_cur, t_nxt, more, araw);
      BRV_STAMP(cyc_stage += stamp_cycles() - tq);
      process_tile(b_cur, t_cur + 32*wm, buf);
      b_cur = b_nxt; t_cur = t_nxt;
    }
#endif
  }
  flush_stats();
  flush_astats();
  if (EM == E_GLN_BWD) {
    // column sums: reduce over the lanes that share a chunk (same lane % CH)
    float ca[8], cb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = (j & 1) ? colA[j >> 1].y : colA[j >> 1].x;
      float y = (j & 1) ? colB[j >> 1].y : colB[j >> 1].x;
#pragma unroll
      for (int off = 32; off >= CH; off >>= 1) {
        x += __shfl_xor(x, off, 64);
        y += __shfl_xor(y, off, 64);
      }
      ca[j] = x; cb[j] = y;
    }
    if (lane < CH) {
      const long long ro = e.n_rep > 1 ? (long long)(blockIdx.x % e.n_rep)*e.rep_stride : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = ncol + j;
        if (n < e.N) {
          atomic_add_f32(e.dgamma + ro + n, ca[j]);
          atomic_add_f32(e.dbeta + ro + n, cb[j]);
        }
      }
    }
  }
#ifdef BRV_DIAG
  if ((dbg & 64) && p.dbg_out && lane == 0) {
    long long* o = p.dbg_out + ((long long)(blockIdx.y*gridDim.x + blockIdx.x)*NW + wid)*4;
    if (wid == 1) {
      const long long r_exit = stamp_realtime();
      o[0] = stamp_cycles() - t_entry; o[1] = r_exit - r_entry; o[2] = r_entry; o[3] = r_exit;
    }
    else if (wid == 2) { o[0] = KP; o[1] = gridDim.x; o[2] = EM; o[3] = t_end - t_begin; }
    else { o[0] = cyc_stage; o[1] = cyc_mfma; o[2] = cyc_epi; o[3] = stamp_cycles() - cyc_total0; }
  }
#endif
}

}  // namespace brv
