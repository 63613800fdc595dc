// The flat Conv-TasNet parameter vector in ConvTasNet.parameters() order, written once
// for the three host drivers: the bf16 path (convtasnet.hip), the fp32 path (ctn_f32.hip) and streaming
// inference (ctn_stream.hip). Host code only: offsets travel to the kernels as plain numbers.
#pragma once
#include <vector>

#include "../../include/brever_hip.h"
#include "status.h"

namespace brv {

// offsets (floats) of one TCN block's tensors; res_w = res_b = -1 in the last block (no residual conv)
struct CtnBlockOff {
  long long conv_w, conv_b, dconv_w, dconv_b, res_w, res_b, skip_w, skip_b,
      n1_g, n1_b, n2_g, n2_b, prelu1, prelu2;
};

// `Blk` is CtnBlockOff or a struct derived from it that adds what one path keeps per block.
template <class Blk>
struct CtnLayout {
  int N, K, Bn, H, Sc, P, layers, nb, S, hop, causal;
  long long enc_w, dec_w, ln_g, ln_b, bott_w, bott_b, tcn_prelu, out_w, out_b, n_params;
  std::vector<Blk> blk;
  std::vector<long long> tensor_offsets;      // start of every tensor, in parameters() order

  // `limits`: the calling path's own range checks (kernel size, widths, ...). They run after the
  // common validation and before any offset is taken, so each path keeps its status codes and messages.
  int init(const brv_ctn_config* c, int (*limits)(const brv_ctn_config*)) {
    if (!c) return fail(-1, "null config");
    if (c->filters < 1 || c->filter_length < 2 || c->bottleneck_channels < 1 ||
        c->hidden_channels < 1 || c->skip_channels < 1 || c->layers < 1 ||
        c->repeats < 1 || c->output_sources < 1)
      return fail(-1, "invalid Conv-TasNet hyper-parameters");
    if (int r = limits(c)) return r;
    N = c->filters; K = c->filter_length; Bn = c->bottleneck_channels;
    H = c->hidden_channels; Sc = c->skip_channels; P = c->kernel_size;
    layers = c->layers; nb = c->layers*c->repeats; S = c->output_sources; hop = K/2; causal = c->causal != 0;
    long long o = 0;
    auto take = [&](long long n) { tensor_offsets.push_back(o); long long r = o; o += n; return r; };
    enc_w = take((long long)N*K);
    dec_w = take((long long)N*K);
    ln_g = take(N); ln_b = take(N);
    bott_w = take((long long)Bn*N); bott_b = take(Bn);
    blk.resize(nb);
    for (int i = 0; i < nb; ++i) {
      CtnBlockOff& b = blk[i];
      b.conv_w = take((long long)H*Bn); b.conv_b = take(H);
      b.dconv_w = take((long long)H*P); b.dconv_b = take(H);
      if (i < nb - 1) { b.res_w = take((long long)Bn*H); b.res_b = take(Bn); }
      else { b.res_w = -1; b.res_b = -1; }
      b.skip_w = take((long long)Sc*H); b.skip_b = take(Sc);
      b.n1_g = take(H); b.n1_b = take(H); b.n2_g = take(H); b.n2_b = take(H);
      b.prelu1 = take(1); b.prelu2 = take(1);
    }
    tcn_prelu = take(1);
    out_w = take((long long)S*N*Sc); out_b = take((long long)S*N);
    n_params = o;
    return 0;
  }

  // frames of an input of L samples: Encoder.pad (convtasnet.py:115-120) pads at the end to a whole hop
  long long frames(long long L) const {
    const long long pad = ((K - L) % hop + hop) % hop;     // Python modulo
    const long long Lp = L + pad;
    return Lp < K ? 0 : (Lp - K)/hop + 1;
  }
};

// the common validation leaves kernel_size to the paths; two of them refuse < 1 with its status and words
inline int ctn_kernel_size_positive(const brv_ctn_config* c) {
  return c->kernel_size < 1 ? fail(-1, "invalid Conv-TasNet hyper-parameters") : 0;
}

}  // namespace brv
