"""The shared host ops of the models (brever_amd/models/_ops.py) without a device: the one ``use_amp`` flag, the
entry point ``gemm`` picks for each combination of dtypes and switches, and the rule that model files share code
through ``_ops`` only. The library is stubbed; CPU tensors stand in, so only dtypes, strides and alignment matter."""
import ast
import os
import types

import pytest
import torch

from brever_amd import hip
from brever_amd.models import _ops, dccrn, sgmse_train

MODELS = os.path.dirname(os.path.abspath(_ops.__file__))


def test_one_amp_flag_under_every_name_and_amp_restores_it():
    assert dccrn._AMP is sgmse_train.AMP is _ops.AMP
    assert _ops.AMP == {'on': False}
    with _ops.amp(1):
        assert _ops.AMP['on'] is True
    assert _ops.AMP['on'] is False
    with pytest.raises(KeyError):
        with _ops.amp(True):
            raise KeyError('inside')
    assert _ops.AMP['on'] is False
    with _ops.amp(False):
        assert _ops.AMP['on'] is False


@pytest.fixture
def calls(monkeypatch):
    """Every library call ``gemm`` makes, as (name, args); the size rules of the narrow-layer kernels answer like the
    library does for K, N <= 64."""
    log = []
    lib = types.SimpleNamespace(
        brv_linear_small_supported=lambda M, N, K: int(N <= 64 and K <= 64),
        brv_linear_small_wgrad_supported=lambda rows, M, N: int(M <= 64 and N <= 64),
        brv_linear_small_wgrad_scratch_bytes=lambda M, N: 4*M*N)
    monkeypatch.setattr(hip, 'lib', lambda: lib)
    monkeypatch.setattr(hip, 'stream', lambda: 'stream')
    monkeypatch.setattr(hip, 'call', lambda name, *args: log.append((name, args)))
    monkeypatch.setattr(hip, 'gemm_f32', lambda *args: log.append(('hip.gemm_f32', args)))
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(_ops, '_SMALL_SCRATCH', {})
    return log


def _mat(rows, cols, dtype=torch.float32):
    t = torch.zeros(rows, cols, dtype=dtype)
    assert t.data_ptr() % 16 == 0
    return t


def test_gemm_dispatch_table(calls):
    f32, bf16 = torch.float32, torch.bfloat16
    M, N, K = 96, 80, 72                        # too wide for the narrow-layer kernels
    dims = (1, M, N, K, K, N, N)

    def run(a=f32, b=f32, d=f32, **kw):
        del calls[:]
        _ops.gemm(_mat(M, K, a), _mat(K, N, b), _mat(M, N, d), *dims, **kw)
        (name, args), = calls
        return name, args

    name, args = run()
    assert name == 'hip.gemm_f32' and len(args) == 20 and args[3:10] == dims and args[-1] == 0 and args[-2] is None
    name, args = run(mode=1)
    assert name == 'hip.gemm_f32' and args[-1] == 1
    name, args = run(workspace=False)
    assert name == 'brv_gemm_f32' and args[3:10] == dims and args[-2:] == (0, 'stream')
    name, args = run(small=True)                # the size rule refuses: the MFMA product
    assert name == 'hip.gemm_f32'
    for kw in ({}, {'workspace': False}):       # (``workspace`` only matters to the exact-fp32 product)
        name, args = run(lowp=True, mode=2, **kw)
        assert name == 'brv_gemm_bf16' and args[-2:] == (2, 'stream')
    for dt, flags in (({'b': bf16}, 1), ({'d': bf16}, 2), ({'a': bf16}, 4), ({'a': bf16, 'b': bf16, 'd': bf16}, 7)):
        name, args = run(lowp=True, mode=1, **dt)
        assert name == 'brv_gemm_bf16_mixed' and args[-3:] == (1, flags, 'stream'), dt
        with pytest.raises(AssertionError):     # bf16 tensors exist under use_amp only
            run(**dt)


def test_gemm_narrow_layer_paths_need_small_and_their_layout(calls):
    rows, I, O = 40, 32, 24
    x, w, y, bias = _mat(rows, I), _mat(O, I), _mat(rows, O), torch.zeros(O)

    def run(*args, **kw):
        del calls[:]
        _ops.gemm(*args, **kw)
        (name, a), = calls
        return name, a

    # y = x @ w^T + bias per column, as TF-GridNet's linear node asks for it
    fwd = (x, w, y, 1, rows, O, I, I, I, O)
    name, a = run(*fwd, trans_b=1, bias=bias, mode=2, small=True)
    assert name == 'brv_linear_small' and a[4:] == (rows, O, I, I, I, O, 1, 0, 'stream') and a[2] is bias
    name, a = run(*fwd, trans_b=1, bias=bias, mode=2, small=True, lowp=True)
    assert name == 'brv_linear_small'          # taken before ``lowp`` is looked at
    name, a = run(*fwd, trans_b=1, bias=bias, mode=2, small=False)
    assert name == 'hip.gemm_f32' and a[-1] == 2
    name, a = run(*fwd, trans_b=1, bias=bias, mode=0, small=True)      # a per-row bias is not the kernel's
    assert name == 'hip.gemm_f32'
    name, a = run(x[:, 1:], w, y, 1, rows, O, I - 1, I, I, O, trans_b=1, small=True)     # a off its 16 bytes
    assert name == 'hip.gemm_f32'
    # dw = dy^T @ x
    dy, dw = _mat(rows, O), _mat(O, I)
    wgrad = (dy, x, dw, 1, O, I, rows, O, I, I)
    name, a = run(*wgrad, trans_a=1, small=True)
    assert name == 'brv_linear_small_wgrad' and a[4:] == (rows, O, I, O, I, I, 'stream')
    assert a[3].dtype == torch.uint8 and a[3].numel() == 4*O*I
    scratch = a[3]
    name, a = run(*wgrad, trans_a=1, small=True)
    assert a[3] is scratch                      # one buffer per (device, stream)
    name, a = run(*wgrad, trans_a=1, small=False)
    assert name == 'hip.gemm_f32'
    name, a = run(*wgrad, trans_a=1, small=True, bias=torch.zeros(O))
    assert name == 'hip.gemm_f32'
    dy2, x2, dw2 = torch.zeros(2, rows, O), torch.zeros(2, rows, I), torch.zeros(2, O, I)
    name, a = run(dy2, x2, dw2, 2, O, I, rows, O, I, I, rows*O, rows*I, O*I, trans_a=1, small=True)
    assert name == 'hip.gemm_f32' and a[3] == 2
    name, a = run(dy2, x2, dw, 1, O, I, rows, O, I, I, trans_a=1, kbatch=2, a_kbs=rows*O, b_kbs=rows*I, small=True)
    assert name == 'hip.gemm_f32'


def test_model_files_share_code_through_ops_only():
    """No model file imports an underscore name from another model file (``_ops`` is where shared pieces live), and
    the matrix-product dispatcher and the (B, features, frames) linear node exist once."""
    files = sorted(f for f in os.listdir(MODELS) if f.endswith('.py'))
    models = {f[:-3] for f in files} - {'_ops', '__init__'}
    gemms = []
    for f in files:
        tree = ast.parse(open(os.path.join(MODELS, f)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module in models:
                private = [a.name for a in node.names if a.name.startswith('_')]
                assert not private, (f, node.module, private)
            if isinstance(node, ast.FunctionDef) and node.name in ('_gemm', 'gemm'):
                gemms.append(f)
            assert not (isinstance(node, ast.ClassDef) and node.name in ('_LinearLowpFunction', '_LinearFunction')), f
    assert gemms == ['_ops.py']
