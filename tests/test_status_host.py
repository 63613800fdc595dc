"""The error contract of include/brever_hip.h on the host: every failing call sets brv_last_error().

No test here needs a device: each call is refused on its arguments before anything is launched.
"""
import ctypes
import glob
import os
import re

import pytest

from brever_amd import hip

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'brever_amd', 'csrc')

# Entry points with a failing path, by translation unit. Each is called with every pointer NULL and every
# count, size and length 0 (a call that wrongly went on would launch over zero elements and touch no memory).
# gemm_f32_big.hip exports nothing: its refusal is reached through brv_gemm_f32 on large products only.
REFUSING_BY_UNIT = {
    'cconv': (
        'brv_cconv_pack', 'brv_cconv_pack_complex', 'brv_cconv_rows', 'brv_cconv_rows_bf16',
        'brv_cconv_rows_ex', 'brv_cconv_wgrad_workspace_bytes', 'brv_cconv_wgrad', 'brv_cconv_wgrad_bf16',
    ),
    'conv_mfma': (
        'brv_conv2d_packed_size', 'brv_conv2d_pack_f16', 'brv_conv2d_mfma_forward',
    ),
    'conv_nhwc': (
        'brv_conv_nhwc_packed_size', 'brv_conv_nhwc_pack', 'brv_groupnorm_fold_chan2', 'brv_conv_nhwc_forward',
        'brv_conv_nhwc_forward_ws', 'brv_conv_nhwc_forward_gn_ws', 'brv_conv_nhwc_forward_gn',
    ),
    'convtasnet': (
        'brv_ctn_param_count', 'brv_ctn_param_tensors', 'brv_ctn_param_offset', 'brv_ctn_frames',
        'brv_ctn_prepared_bytes', 'brv_ctn_workspace_bytes', 'brv_ctn_workspace_offset', 'brv_ctn_prepare',
        'brv_ctn_forward', 'brv_ctn_grad_bucket', 'brv_ctn_backward', 'brv_ctn_backward_part',
    ),
    'ctn_f32': (
        'brv_ctn_f32_workspace_bytes', 'brv_ctn_f32_forward', 'brv_ctn_f32_backward',
        'brv_ctn_f32_backward_part',
    ),
    'ctn_stream': (
        'brv_ctn_stream_state_bytes', 'brv_ctn_stream_workspace_bytes', 'brv_ctn_stream_reset',
        'brv_ctn_stream_tail', 'brv_ctn_stream_step',
    ),
    'dccrn': (
        'brv_conv2d_forward', 'brv_conv_transpose2d_forward', 'brv_batchnorm2d_forward',
        'brv_batchnorm2d_forward_bf16', 'brv_batchnorm2d_forward_bf16io', 'brv_lstm_recurrent_forward',
        'brv_lstm_recurrent_forward_bf16', 'brv_lstm_recurrent_backward_bf16', 'brv_combine',
        'brv_complex_mix_forward', 'brv_complex_mix_backward', 'brv_dccrn_apply_mask',
        'brv_dccrn_apply_mask_batched', 'brv_conv2d_wgrad', 'brv_batchnorm2d_backward',
        'brv_batchnorm2d_backward_bf16', 'brv_batchnorm2d_backward_bf16io', 'brv_batchnorm2d_backward_ex',
        'brv_lstm_recurrent_backward', 'brv_dccrn_apply_mask_backward',
        'brv_dccrn_apply_mask_backward_batched', 'brv_istft_env_divide', 'brv_im2col', 'brv_col2im',
        'brv_im2col_bf16', 'brv_col2im_bf16', 'brv_complex_weight_pack', 'brv_complex_weight_unpack',
        'brv_complex_bias_pack', 'brv_complex_bias_unpack', 'brv_cplx_moments', 'brv_cplx_affine_forward',
        'brv_cplx_affine_backward', 'brv_cplx_moments_backward',
    ),
    'dccrn_stream': (
        'brv_dccrn_stream_state_bytes', 'brv_dccrn_stream_workspace_bytes', 'brv_dccrn_stream_reset',
        'brv_dccrn_stream_step', 'brv_dccrn_stream_tail',
    ),
    'ffnn': (
        'brv_fbe_power', 'brv_compress', 'brv_binaural', 'brv_interaural_coherence', 'brv_col_normalize',
        'brv_deltas', 'brv_irm', 'brv_stack_frames', 'brv_static_norm', 'brv_cumulative_norm',
        'brv_relu_dropout_forward', 'brv_relu_dropout_backward', 'brv_dropout_apply', 'brv_sigmoid_forward',
        'brv_sigmoid_backward', 'brv_row_sum', 'brv_masked_mean_spec',
    ),
    'flac': (
        'brv_flac_info', 'brv_flac_decode', 'brv_flac_encode16',
    ),
    'lstm_tile': (
        'brv_lstm_tile_forward', 'brv_lstm_tile_backward',
    ),
    'nhwc': (
        'brv_nchw_to_nhwc_f16', 'brv_nhwc_f16_to_nchw', 'brv_nhwc_chan_stats', 'brv_groupnorm_fold_chan',
        'brv_nhwc_affine_act', 'brv_nhwc_fir_resample2d', 'brv_nhwc_fir_resample2d_dual', 'brv_nhwc_axpby',
        'brv_nhwc_conv1x1_packed_size', 'brv_nhwc_conv1x1_pack', 'brv_nhwc_conv1x1_forward',
        'brv_nhwc_conv3x3_small_pack', 'brv_nhwc_conv3x3_small', 'brv_nhwc_add_pointwise',
    ),
    'norm': (
        'brv_causal_groupnorm_forward', 'brv_causal_groupnorm_backward',
    ),
    'ops': (
        'brv_snr_forward', 'brv_snr_forward_strided', 'brv_snr_backward', 'brv_snr_backward_strided',
        'brv_sisnr_forward', 'brv_sisnr_backward', 'brv_mse_backward', 'brv_mse_forward', 'brv_apply_mask',
        'brv_l1_forward', 'brv_l1_backward', 'brv_mag_l1_forward', 'brv_mag_l1_backward', 'brv_clip_adam_step',
        'brv_clip_adam_step2', 'brv_memset_zero', 'brv_mean_f32', 'brv_ema_update', 'brv_si_scale_forward',
        'brv_si_scale_backward',
    ),
    'sgmse': (
        'brv_groupnorm_fold', 'brv_affine_act', 'brv_groupnorm_backward', 'brv_affine_act_backward',
        'brv_silu_backward', 'brv_softmax_rows_backward', 'brv_silu', 'brv_softmax_rows', 'brv_fir_resample2d',
        'brv_axpby', 'brv_fourier_features',
    ),
    'stft': (
        'brv_stft_frames', 'brv_stft_forward', 'brv_istft_backward', 'brv_stft_adjoint',
        'brv_framed_dft_forward', 'brv_framed_dft_transpose', 'brv_gemm_f32', 'brv_gemm_f32_ws',
        'brv_gemm_bf16_mixed', 'brv_gemm_bf16_conv', 'brv_gemm_bf16', 'brv_dft64_forward',
        'brv_dft64_synthesis', 'brv_overlap_add', 'brv_pad_signal', 'brv_polar', 'brv_mag_phase',
        'brv_spec_compress', 'brv_spec_compress_backward', 'brv_matmul_f32',
    ),
    'stoi': (
        'brv_resample_poly', 'brv_stoi_compact', 'brv_stoi_bands', 'brv_stoi_correlate',
    ),
    'tfgridnet': (
        'brv_head_permute', 'brv_rownorm_forward', 'brv_rownorm_backward', 'brv_col_sum', 'brv_linear_small',
        'brv_linear_small_wgrad', 'brv_col_sum_bf16', 'brv_row_std', 'brv_row_scale',
    ),
}
# the two whose checks accept 0: position of the count that takes a negative value instead
NEGATIVE_COUNT = {'brv_nhwc_axpby': (5, -8), 'brv_memset_zero': (1, -1)}

# Exports with no failing path at all, each with its reason.
NO_REFUSAL = {
    'brv_version': 'a constant',
    'brv_last_error': 'reads the message',
    'brv_prof_create': 'allocates a host object, returns the handle',
    'brv_prof_collect': 'returns the byte count needed; a NULL handle gives 0',
    'brv_prof_destroy': 'returns nothing',
    'brv_cconv_packed_bytes': 'size arithmetic only',
    'brv_lstm_recurrent_bf16_supported': 'flag query',
    'brv_lstm_tile_supported': 'flag query',
    'brv_lstm_tile_variant': 'flag query',
    'brv_head_permute_supported': 'flag query',
    'brv_linear_small_supported': 'flag query',
    'brv_linear_small_wgrad_supported': 'flag query',
    'brv_linear_small_wgrad_scratch_bytes': 'size arithmetic only',
    'brv_rownorm_scratch_bytes': 'size arithmetic only',
    'brv_col_sum_scratch_bytes': 'size arithmetic only',
    'brv_causal_groupnorm_scratch_bytes': 'size arithmetic only',
    'brv_groupnorm_scratch_bytes': 'size arithmetic only',
    'brv_loss_scratch_bytes': 'size arithmetic only',
    'brv_stoi_frames': 'frame count, 0 for a short signal',
    'brv_gemm_f32_workspace_bytes': 'size query: 0 means "no workspace needed"',
    'brv_conv_nhwc_split_ws_bytes': 'size query: 0 means "no workspace needed"',
}


def _zeros(name):
    args = [None if a in (hip._c_ptr, ctypes.c_char_p) else 0 for a in hip.SIGNATURES[name][1]]
    if name in NEGATIVE_COUNT:
        pos, value = NEGATIVE_COUNT[name]
        args[pos] = value
    return tuple(args)


REFUSING = {name: _zeros(name) for names in REFUSING_BY_UNIT.values() for name in names}
# every refusal of an argument is -1 (the header's "invalid argument"); none of these reaches a -2
EXPECTED_CODE = -1


def _last_error():
    msg = hip.lib().brv_last_error()
    return msg.decode() if msg else ''


def test_every_export_refuses_or_cannot_fail():
    assert not set(REFUSING) & set(NO_REFUSAL)
    assert set(REFUSING) | set(NO_REFUSAL) == set(hip.SIGNATURES), \
        (set(REFUSING) | set(NO_REFUSAL)) ^ set(hip.SIGNATURES)
    assert sum(len(v) for v in REFUSING_BY_UNIT.values()) == len(REFUSING)      # no name listed twice
    for name in NO_REFUSAL:
        restype, argtypes = hip.SIGNATURES[name]
        # an int status next to pointer arguments (a stream among them) is an entry point that can fail
        assert not (restype is ctypes.c_int and hip._c_ptr in argtypes), name


def test_the_silent_units_are_all_covered():
    silent = {'dccrn', 'cconv', 'stft', 'ffnn', 'ops', 'sgmse', 'nhwc', 'conv_nhwc', 'conv_mfma', 'norm',
              'tfgridnet', 'lstm_tile', 'stoi', 'flac'}      # + gemm_f32_big, which exports nothing
    assert silent <= set(REFUSING_BY_UNIT)
    units = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CSRC, '*.hip'))}
    assert set(REFUSING_BY_UNIT) | {'gemm_f32_big', 'status'} == units


@pytest.mark.parametrize('unit', sorted(REFUSING_BY_UNIT))
def test_a_refusal_overwrites_an_older_message(unit):
    lib = hip.lib()
    for name in REFUSING_BY_UNIT[unit]:
        # re-arm a sentinel with a known text, from another call than the one under test
        assert lib.brv_ctn_param_count(None) == -1
        sentinel = _last_error()
        assert sentinel == 'null config'
        status = getattr(lib, name)(*REFUSING[name])
        msg = _last_error()
        assert status == EXPECTED_CODE, (name, status, msg)
        assert msg, name
        if unit in ('convtasnet', 'ctn_f32', 'ctn_stream', 'dccrn_stream'):
            # these refuse a NULL config in the sentinel's own words: show the overwrite from another text
            assert lib.brv_combine(None, None, None, 0, 0.0, None) == -1
            assert _last_error() == 'requires n >= 1'
            assert getattr(lib, name)(*REFUSING[name]) == EXPECTED_CODE
            assert _last_error() == msg, name
        else:
            assert msg != sentinel, name


def test_flac_codes_keep_their_value_and_gain_a_message():
    lib = hip.lib()
    junk = b'not a flac stream' + bytes(64)
    assert lib.brv_ctn_param_count(None) == -1
    assert lib.brv_flac_info(junk, len(junk), None, None, None, None) == -10
    assert _last_error() == 'malformed FLAC stream: decoder code -10'


def _sources():
    paths = [p for ext in ('*.hip', '*.cuh', '*.h') for p in glob.glob(os.path.join(CSRC, ext))]
    assert len(paths) > 30
    return {os.path.basename(p): open(p).read() for p in paths}


def test_one_definition_of_each_helper():
    src = _sources()
    text = '\n'.join(src.values())
    assert text.count('#define GRID_STRIDE') == 1
    assert text.count('flat_grid(long long') == 1
    assert '_OK(expr) do {' not in text
    assert 'brv_internal_set_error' not in text
    assert len(re.findall(r'#define \w*_OK\w*\(', text)) == 1          # BRV_HIP_OK
    assert len(re.findall(r'thread_local std::string', text)) == 1
    for name, s in src.items():
        if name.endswith('.hip'):
            assert '#include "status.h"' in s, name


def test_no_refusal_without_a_message():
    # flac.hip: the decoder's internal helpers return their own codes (-10 ... -51); the entry points turn
    # them into a message (test_flac_codes_keep_their_value_and_gain_a_message).
    for name, s in _sources().items():
        if name == 'flac.hip':
            continue
        for n, line in enumerate(s.split('\n'), 1):
            if re.search(r'return -[123];', line):
                # the size queries of Conv-TasNet: Layout::init has set the message
                assert re.search(r'if \(l\.init\(cfg\)\) return -1;', line), f'{name}:{n}: {line.strip()}'
            assert not re.search(r'return \(int\)hipGetLastError\(\);', line), f'{name}:{n}'
