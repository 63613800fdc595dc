/* brever_ffnn_stream.h -- C ABI of libbrever_ffnn_stream.so: the MI355X (gfx950) kernels of stateful streaming
 * inference of the FFNN mask estimator (brever_amd/streaming.py: FFNNStreamer; brever/models/ffnn/ffnn.py).
 *
 * A library of its own next to libbrever_hip.so, with the same conventions (include/brever_hip.h):
 *   - every pointer is a device pointer borrowed from the caller (the config struct itself is host memory);
 *     the library allocates nothing and keeps no process-global state;
 *   - every call takes the HIP stream to launch on and never synchronises;
 *   - return value: 0 ok, -1 refused argument, -2 unsupported configuration, > 0 a hipError_t;
 *     brv_ffs_last_error() gives the thread-local message every non-zero return has set.
 *
 * One call advances n streams by `hops` hops; its columns are the (stream, frame) pairs. The two 512-point
 * transforms of a call are brv_dft64_forward / brv_dft64_synthesis of the main library with the tables of the
 * offline STFT, called by the host between the three launches groups below, so a streamed spectrum is the
 * offline one frame for frame:
 *
 *     brv_ffs_step_frames   carry | chunk, both channels                    -> xin   (n channels, lag + hops hop)
 *     brv_dft64_forward     frames = hops, pad_left = 0                     -> spec  (n channels, bins, hops) complex
 *     brv_ffs_step_net      power, mel, compression, stacking, normaliser,
 *                           the MLP, mel-to-bin mask x channel-mean spectrum -> mspec (n, bins, hops) complex
 *     brv_dft64_synthesis                                                   -> frames (n, hops, n_fft)
 *     brv_ffs_step_emit     overlap-add, envelope, output; state commit     -> y
 *
 * With d = n_fft / (2 hop) - 1, the frame of hop h of a stream is STFT frame t = h - d of the centred offline
 * transform (frames t < 0 do not exist; in a tail neither do frames behind the last one of the right-padded
 * signal), and the output of hop h is samples [h hop - lag, (h + 1) hop - lag), lag = n_fft - hop: zeros
 * before sample 0. Every state read of a call precedes every state write: the only kernel that writes state
 * is the last launch of brv_ffs_step_emit, which copies from the workspace.
 */
#ifndef BREVER_FFNN_STREAM_H
#define BREVER_FFNN_STREAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

#define BRV_FFS_MAX_HIDDEN 8         /* hidden layers; linear layers = hidden + 1 */
#define BRV_FFS_MAX_FEATURES 6       /* the non-DCT members of the fbe family */

/* Geometry of an FFNN and the addresses its values live at (read at every call).
 * Features, in the order FeatureExtractor concatenates them: feat_norm[i] = 1 divides a frame's mel energies by
 * their sum + eps_feat ('pdf'), feat_comp[i] = 0 none, 1 log(x + eps_feat), 2 cube root. The stacked input
 * has rows = (stacks + 1) features mel rows. norm = 0: (x - mean[row]) / std[row]; norm = 1: cumulative
 * mean / variance over the frames so far in fp64, eps_norm under the root. widths[l] = outputs of linear
 * layer l = 0 .. hidden (the last one = mel); weight[l] (widths[l], widths[l - 1]) row-major, bias[l].
 * mel_fwd (mel, bins) and mel_inv (bins, mel) are MelFilterbank.filters and .inverse_filters.
 * The STFT must be the one FFNN builds: n_fft == frame_length, centred, constant padding, normalised,
 * one-sided, no compression, scale 1, and frame_length % (2 hop) == 0 (-2 otherwise).
 * Limits (-2 beyond them): hidden <= 8, n_fft <= 4096, mel <= 256, channels <= 8, stacks <= 64. */
typedef struct brv_ffs_config {
  int32_t n_fft, frame_length, hop, channels;
  int32_t center, pad_constant, normalized, onesided;
  float compression, scale;
  int32_t mel, stacks, features, norm;
  int32_t feat_norm[BRV_FFS_MAX_FEATURES], feat_comp[BRV_FFS_MAX_FEATURES];
  float eps_feat, eps_norm;
  int32_t hidden, reserved;
  int32_t widths[BRV_FFS_MAX_HIDDEN + 1];
  int32_t reserved2;
  const float* weight[BRV_FFS_MAX_HIDDEN + 1];
  const float* bias[BRV_FFS_MAX_HIDDEN + 1];
  const float* mean;
  const float* std;
  const float* mel_fwd;
  const float* mel_inv;
} brv_ffs_config;

int brv_ffs_version(void);
const char* brv_ffs_last_error(void);

/* Bytes of one stream slot (slot i at byte i * state_bytes of the caller's buffer; layout in DESIGN.md 5g)
 * and of the workspace of a call of n streams x hops hops (a tail: hops = n_fft / hop). */
int64_t brv_ffs_state_bytes(const brv_ffs_config* cfg);
int64_t brv_ffs_workspace_bytes(const brv_ffs_config* cfg, int64_t n, int64_t hops);

/* Put the n slots listed in ids (int32, on the device, each in [0, slots): others are skipped) back to the
 * start of a stream. */
int brv_ffs_reset(const brv_ffs_config* cfg, void* state, int64_t slots, const int32_t* ids, int64_t n,
                  brv_stream_t stream);

/* The three launch groups of a call. rest < 0: a step, x (n, channels, hops hop) fp32 -> y (n, hops hop).
 * rest = r >= 0: the tail of streams that end, x (n, channels, r) their last r < hop samples (NULL if r = 0),
 * hops = n_fft / hop, y (n, lag + r) the samples still owed; a tail commits nothing: reset the slots next. */
int brv_ffs_step_frames(const brv_ffs_config* cfg, const void* state, int64_t slots, const int32_t* ids,
                        int64_t n, const float* x, int64_t hops, int64_t rest, float* xin, brv_stream_t stream);
int brv_ffs_step_net(const brv_ffs_config* cfg, const void* state, int64_t slots, const int32_t* ids, int64_t n,
                     int64_t hops, int64_t rest, const float* spec, float* mspec, void* workspace,
                     int64_t workspace_bytes, brv_stream_t stream);
int brv_ffs_step_emit(const brv_ffs_config* cfg, const float* window, void* state, int64_t slots,
                      const int32_t* ids, int64_t n, int64_t hops, int64_t rest, const float* xin,
                      const float* frames, float* y, void* workspace, int64_t workspace_bytes,
                      brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
