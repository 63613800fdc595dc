"""Pins the ORACLE (oracle/*.py, the CPU restatement used as checker) against
golden vectors generated from the imported reference, and -- through the
reference's own 2-epoch training golden -- pins the host-side trainer, sampler
and collate code at the same time. CPU only."""
import json
import os
import random
import tempfile

import numpy as np
import pytest
import torch

from oracle import criterion as oc
from oracle.convtasnet import OracleConvTasNet

from helpers import DummyDataset, DummyModel


def load_flat(model, flat):
    off = 0
    with torch.no_grad():
        for p in model.parameters():
            n = p.numel()
            p.copy_(torch.from_numpy(flat[off:off + n]).view(p.shape))
            off += n
    assert off == flat.size


def test_losses_match_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, 'losses.npz'))
    x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    lengths = torch.from_numpy(g['lengths'])
    for name in ['snr', 'sisnr', 'mse']:
        got = oc.CRITERIA[name](x, y, lengths)
        assert torch.allclose(got, torch.from_numpy(g[name]), rtol=1e-5, atol=1e-6), name
    got = oc.mse(x, y, lengths, weight=torch.from_numpy(g['weight']))
    assert torch.allclose(got, torch.from_numpy(g['mse_weighted']), rtol=1e-5, atol=1e-7)
    xg = x.clone().requires_grad_(True)
    oc.snr(xg, y, lengths).mean().backward()
    assert torch.allclose(xg.grad, torch.from_numpy(g['snr_grad']), rtol=1e-4, atol=1e-8)


def test_multiresyu_matches_reference(golden_dir):
    """MultiResYuLoss values and gradients (default and 3 resolutions) vs the reference."""
    g = np.load(os.path.join(golden_dir, 'losses.npz'))
    x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    lengths = torch.from_numpy(g['lengths'])
    gw = torch.from_numpy(g['gweight'])
    for tag, kw in (('multiresyu', {}),
                    ('multiresyu3', dict(frame_lengths=[512, 256, 128], time_domain_weight=0.3,
                                         spectral_weight=0.7)),
                    ('multiresyu_si', dict(frame_lengths=[256, 128], scale_invariant=True))):
        xg = x.clone().requires_grad_(True)
        got = oc.multiresyu(xg, y, lengths, **kw)
        assert torch.allclose(got, torch.from_numpy(g[tag]), rtol=1e-5, atol=1e-6), tag
        (got*gw).sum().backward()
        assert torch.allclose(xg.grad, torch.from_numpy(g[tag + '_grad']), rtol=1e-4,
                              atol=1e-7), tag


@pytest.mark.parametrize('name', ['snr', 'sisnr', 'mse'])
def test_losses_batched_equals_per_item(name):
    """The reference's own property test (tests/test_losses.py:13-57)."""
    torch.manual_seed(0)
    B, S, lo, hi = 5, 3, 300, 900
    lengths = torch.randint(lo, hi, (B,))
    x = torch.randn(B, S, hi)
    y = torch.randn(B, S, hi)
    for b in range(B):
        y[b, :, lengths[b]:] = 0
    batched = oc.CRITERIA[name](x, y, lengths)
    single = torch.stack([
        oc.CRITERIA[name](x[b:b+1, :, :lengths[b]], y[b:b+1, :, :lengths[b]],
                          lengths[b:b+1])[0] for b in range(B)])
    assert torch.allclose(batched, single, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('tag', ['small', 'small2', 'causal', 'causal2'])
def test_convtasnet_forward_backward_match_reference(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, f'convtasnet_{tag}.npz'))
    model = OracleConvTasNet(**json.loads(str(g['config'])))
    load_flat(model, g['params'])
    batch = torch.from_numpy(g['batch'])
    lengths = torch.from_numpy(g['lengths'])
    out = model(batch[:, 0])
    assert torch.allclose(out, torch.from_numpy(g['output']), rtol=1e-5, atol=1e-6)
    loss = model.loss(batch, lengths, use_amp=False)
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-5
    loss.backward()
    grads = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    ref = torch.from_numpy(g['grads'])
    assert torch.allclose(grads, ref, rtol=1e-4, atol=1e-6), (grads - ref).abs().max()


def test_default_init_and_forward_match_reference(golden_dir):
    """Seeded construction consumes the RNG in the reference's order, so the
    4 935 217 default parameters (343 tensors) reproduce exactly."""
    g = np.load(os.path.join(golden_dir, 'convtasnet_default.npz'))
    torch.manual_seed(0)
    model = OracleConvTasNet()
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert flat.numel() == 4_935_217 and len(model.state_dict()) == 343
    assert np.array_equal(flat[:64].numpy(), g['first_params'])
    assert abs(float(flat.double().sum()) - float(g['param_sum'])) < 1e-6
    assert abs(float(flat.double().abs().sum()) - float(g['param_abs_sum'])) < 1e-6
    batch = torch.from_numpy(g['batch'])
    out = model(batch[:, 0])
    assert torch.allclose(out, torch.from_numpy(g['output']), rtol=1e-4, atol=1e-6)
    loss = model.loss(batch, torch.from_numpy(g['lengths']), use_amp=False)
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-4
    loss.backward()
    gn = torch.stack([p.grad.norm() for p in model.parameters()])
    assert torch.allclose(gn, torch.from_numpy(g['grad_norms']), rtol=2e-3, atol=1e-7)
    # the product model shares the construction order (same seeded parameters)
    from brever_amd.models import ConvTasNet
    torch.manual_seed(0)
    prod = ConvTasNet()
    assert torch.equal(prod.flat_params(), flat)
    assert list(prod.state_dict().keys()) == list(model.state_dict().keys())


@pytest.mark.parametrize('ema', [False, True])
@pytest.mark.parametrize('tag', ['dummy', 'convtasnet'])
def test_training_flow_reproduces_reference_golden(golden_dir, tag, ema):
    """Reference tests/test_training.py:34-45,83-94: 8 s dynamic bucket batches,
    2 epochs, Adam (+ clip 5.0 for Conv-TasNet), EMA on, CPU. The literals in the
    reference test file equal the fixture (checked when it was generated).

    The fixture was recorded with a no-op stand-in for the absent ``torch_ema``
    wheel, so its *validation* losses are those of the raw weights: they are
    compared with ema=False; with ema=True only the trained parameters (which EMA
    never influences) are."""
    from brever_amd.training import BreverTrainer
    g = np.load(os.path.join(golden_dir, 'training.npz'))
    FS = 16000
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    if tag == 'dummy':
        model = DummyModel(channels=2, output_sources=2)
    else:
        model = OracleConvTasNet(
            filters=4, filter_length=2, bottleneck_channels=1, hidden_channels=1,
            skip_channels=1, kernel_size=1, layers=1, repeats=1, output_sources=2)
    train = DummyDataset(16, 3, 2, int(FS*0.5), FS*4, transform=model.transform)
    val = DummyDataset(4, 3, 2, int(FS*0.5), FS*4)

    def make(epochs, tmp):
        return BreverTrainer(
            model=model, train_dataset=train, val_dataset=val, model_dirpath=tmp,
            epochs=epochs, val_period=1, val_metrics=set(),
            batch_sampler='bucket', batch_size=8.0, dynamic_batch_size=True,
            ema=ema, device='cpu', preload=True)

    with tempfile.TemporaryDirectory() as tmp:
        trainer = make(2, tmp)
        trainer.run()
        flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
        assert torch.allclose(flat[:10], torch.from_numpy(g[tag]), rtol=1e-5, atol=1e-7), \
            (flat[:10], g[tag])
        tl = np.array([float(d['loss']) for d in trainer.loss_logger.train_loss])
        assert np.allclose(tl, g[tag + '_train_loss'], rtol=1e-5)
        vl = np.array([float(d['loss']) for d in trainer.loss_logger.val_loss])
        if not ema:
            assert np.allclose(vl, g[tag + '_val_loss'], rtol=1e-5)
        assert os.path.exists(os.path.join(tmp, 'losses.npz'))
        # resume from the checkpoint for one more epoch (reference :303-321)
        train.preloaded_data = None
        val.preloaded_data = None
        trainer = make(3, tmp)
        trainer.run()
        assert trainer.epochs_ran == 3
        again = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
        assert not torch.allclose(flat[:10], again[:10])


def test_stft_oracle_matches_reference(golden_dir):
    """oracle/stft.py (framed rFFT restatement) vs the reference STFT wrapper."""
    import scipy.signal
    from oracle import stft as ost
    g = np.load(os.path.join(golden_dir, 'stft.npz'))
    w = scipy.signal.get_window('hann', 512)
    x = g['x']
    for i, (hop, comp, scale, norm) in enumerate(g['combos']):
        X = ost.stft(x, w, int(hop), bool(norm), comp, scale)
        assert X.shape == g[f'spec{i}'].shape
        assert np.abs(X - g[f'spec{i}']).max() <= 2e-5*np.abs(g[f'spec{i}']).max()
        y = ost.istft(g[f'spec{i}'], w, int(hop), bool(norm), comp, scale)
        assert y.shape == g[f'back{i}'].shape
        assert np.abs(y - g[f'back{i}']).max() <= 1e-5
        assert np.abs(y[..., :4096] - x).max() <= 1e-5          # round trip
    X = ost.stft(g['x_odd'], w, 128)
    assert np.abs(X - g['spec_odd']).max() <= 2e-5*np.abs(g['spec_odd']).max()
    assert ost.istft(g['spec_odd'], w, 128).shape == g['back_odd'].shape == (3072,)
    for hop in (128, 256):
        got = [ost.stft_frames(int(n), 512, hop) for n in g['lens']]
        assert got == list(g[f'frames{hop}'])                 # integer, bit-exact
    assert ost.stft_frames(64000, 512, 128) == 501


def test_conv_stft_oracle_matches_reference(golden_dir):
    """oracle/stft.py conv_stft / conv_istft vs the reference ConvSTFT (3 combos)."""
    import scipy.signal
    from oracle import stft as ost
    g = np.load(os.path.join(golden_dir, 'stft.npz'))
    x = g['x_odd'][None]
    for i, (n, hop, comp, scale, norm) in enumerate(g['conv_combos']):
        w = scipy.signal.get_window('hann', int(n))**0.5
        X = ost.conv_stft(x, w, int(hop), bool(norm), comp, scale)
        ref = g[f'conv_spec{i}']
        assert X.shape == ref.shape
        assert np.abs(X - ref).max() <= 2e-5*np.abs(ref).max()
        y = ost.conv_istft(ref, w, int(hop), bool(norm), comp, scale)
        assert y.shape == g[f'conv_back{i}'].shape
        assert np.abs(y - g[f'conv_back{i}']).max() <= 2e-5*np.abs(g[f'conv_back{i}']).max()


def test_mel_filterbank_and_frame_count_bit_exact(golden_dir):
    """Host-side constants of the product modules: mel matrix and frame arithmetic."""
    from brever_amd import hip
    from brever_amd.modules import STFT, MelFilterbank
    g = np.load(os.path.join(golden_dir, 'stft.npz'))
    mel = MelFilterbank()
    assert np.array_equal(mel.filters.numpy(), g['mel_filters'])
    assert np.array_equal(mel.fc.numpy(), g['mel_fc'])
    assert np.array_equal(mel.scaling.numpy(), g['mel_scaling'])
    for hop in (128, 256):
        got = [hip.lib().brv_stft_frames(int(n), 512, hop) for n in g['lens']]
        assert got == list(g[f'frames{hop}'])
        s = STFT(512, hop)
        assert [s.frame_count(int(n)) + 512//hop for n in g['lens']] == got
    assert STFT(512, 128, onesided=False).bins == 512 and STFT(400, 160, n_fft=512).bins == 257
    with pytest.raises(ValueError):
        STFT(512, 128, pad_mode='mirror')
    with pytest.raises(ValueError):
        STFT(512, 128, n_fft=256)


def _load_oracle_ffnn(g):
    from oracle.ffnn import OracleFFNN
    net = OracleFFNN(hidden_layers=(96, 80), dropout=0.0)
    flat = torch.from_numpy(g['params'])
    o = 0
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(flat[o:o + p.numel()].view_as(p))
            o += p.numel()
        net.mean.copy_(torch.from_numpy(g['mean']))
        net.std.copy_(torch.from_numpy(g['std']))
    return net


def test_ffnn_oracle_matches_reference(golden_dir):
    """transform / forward / loss / gradients / enhance of the reference FFNN at fixed
    weights (fixture from the imported reference, dropout 0)."""
    from oracle.ffnn import OracleFFNN
    g = np.load(os.path.join(golden_dir, 'ffnn.npz'))
    assert sum(p.numel() for p in OracleFFNN().parameters()) == int(g['n_params_default'])
    net = _load_oracle_ffnn(g)
    item = net.transform(torch.from_numpy(g['sources']))
    assert torch.allclose(item, torch.from_numpy(g['item']), rtol=1e-4, atol=1e-5)
    batch, lengths = torch.from_numpy(g['batch']), torch.from_numpy(g['lengths'])
    net.train()
    out = net(batch[:, :384])
    assert torch.allclose(out, torch.from_numpy(g['output']), rtol=1e-5, atol=1e-6)
    loss = net.loss(batch, lengths)
    assert abs(float(loss) - float(g['loss'])) <= 1e-6
    loss.backward()
    grads = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.allclose(grads, torch.from_numpy(g['grads']), rtol=1e-4, atol=1e-8)
    net.eval()
    with torch.no_grad():
        y = net.enhance(torch.from_numpy(g['enhance_in']))
    assert torch.allclose(y, torch.from_numpy(g['enhance_out']), rtol=1e-4, atol=1e-6)


def _load_flat(model, flat):
    o = 0
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.from_numpy(flat[o:o + p.numel()]).view(p.shape))
            o += p.numel()
    assert o == len(flat)


def test_dccrn_oracle_matches_reference(golden_dir):
    """oracle/dccrn.py vs the imported reference: parameter count, forward in train mode
    (batch statistics and the running estimates it leaves behind) and in eval mode."""
    from oracle.dccrn import OracleDCCRN
    g = np.load(os.path.join(golden_dir, 'dccrn.npz'))
    assert sum(p.numel() for p in OracleDCCRN().parameters()) == int(g['n_params_default'])
    net = OracleDCCRN(**json.loads(str(g['config'])))
    _load_flat(net, g['params'])
    x = torch.from_numpy(g['x'])
    net.train()
    with torch.no_grad():
        y = net(x)
    assert torch.allclose(y, torch.from_numpy(g['out_train']), rtol=1e-4, atol=1e-6)
    running = torch.cat([b.reshape(-1).float() for n, b in net.named_buffers() if 'running' in n])
    assert torch.allclose(running, torch.from_numpy(g['running']), rtol=1e-5, atol=1e-7)
    # loss (snr) and gradients, second train-mode call
    from oracle.criterion import snr
    batch, lengths = torch.from_numpy(g['batch']), torch.from_numpy(g['lengths'])
    loss = snr(net(batch[:, 0]), batch[:, 1], lengths).mean()
    assert abs(float(loss) - float(g['loss'])) <= 1e-5
    loss.backward()
    grads = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.allclose(grads, torch.from_numpy(g['grads']), rtol=2e-3, atol=1e-5)
    net.eval()
    with torch.no_grad():
        y = net(x)
    assert torch.allclose(y, torch.from_numpy(g['out_eval']), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('tag', ['pc', 'edm', 'res'])
def test_sgmse_oracle_matches_reference(golden_dir, tag):
    """oracle/sgmse.py vs the imported reference: the preconditioned denoiser at one noise
    level and a full ``enhance`` with the recorded Gaussian draws replayed."""
    from helpers import sgmse_case
    from oracle import sgmse as osg
    g = np.load(os.path.join(golden_dir, 'sgmse.npz'))
    model, net, sde, kw, sampler, window, _ = sgmse_case(g, tag)
    x, y = torch.from_numpy(g[f'{tag}_den_x']), torch.from_numpy(g[f'{tag}_den_y'])
    t = torch.from_numpy(g[f'{tag}_den_t'])
    with torch.no_grad():
        d = osg.denoise(net, sde, x, y, sde.sigma(t), t, **kw)
    ref = torch.from_numpy(g[f'{tag}_den_out'])
    assert (d - ref).abs().max() <= 1e-5*ref.abs().max()
    if tag == 'res':
        return
    with torch.no_grad():
        out = osg.enhance(net, sde, torch.from_numpy(g[f'{tag}_wav']), window, 16, sampler)
    ref = torch.from_numpy(g[f'{tag}_enhance'])
    assert (out - ref).abs().max() <= 1e-4*ref.abs().max()


@pytest.mark.parametrize('tag', ['pc', 'res', 'edm'])
def test_sgmse_training_oracle_matches_reference(golden_dir, tag):
    """The training objective and ALL parameter gradients of the oracle network vs the imported
    reference with the draws of t and of the noise fixed."""
    from helpers import sgmse_case
    from oracle import sgmse as osg
    g = np.load(os.path.join(golden_dir, 'sgmse.npz'))
    model, _, sde, kw, _, _, _ = sgmse_case(g, tag)
    net = osg.Net(model.state_dict(), 'model.net.', skip_scale=0.5**0.5,
                  block_type='adm' if tag == 'edm' else 'ncsn', requires_grad=True)
    loss = osg.train_loss(net, sde, torch.from_numpy(g[f'{tag}_train_batch']),
                          torch.from_numpy(g[f'{tag}_train_lengths']),
                          torch.from_numpy(g[f'{tag}_train_t']),
                          torch.from_numpy(g[f'{tag}_train_noise']), **kw)
    assert abs(float(loss) - float(g[f'{tag}_train_loss'])) <= 1e-5
    loss.backward()
    names = [n[len('model.net.'):] for n, _ in model.named_parameters()]
    got = torch.cat([net.sd[n].grad.reshape(-1) if net.sd[n].grad is not None
                     else torch.zeros(net.sd[n].numel()) for n in names])
    gold = torch.from_numpy(g[f'{tag}_train_grads'])
    assert (got - gold).norm() <= 1e-4*gold.norm()


def test_features_oracle_matches_reference(golden_dir):
    """oracle/features.py vs the imported reference for every feature except 'ic'."""
    from oracle import features as of
    from oracle.ffnn import mel_filters
    g = np.load(os.path.join(golden_dir, 'features.npz'))
    filters = mel_filters()[0] if isinstance(mel_filters(), tuple) else mel_filters()
    filters = np.asarray(filters, dtype=np.float64)
    spec = g['spec'].astype(np.complex128)
    for name in g['names']:
        want = g[str(name)]
        got = of.FEATURES[str(name)](spec, filters)
        scale = np.abs(want).max()
        assert np.abs(got - want).max() <= 2e-4*scale, (name, np.abs(got - want).max(), scale)


# the literals of the reference's own known-answer test for the default SGMSE+ network
# (tests/test_models.py:126-146: every parameter 1e-3, seeded Fourier frequencies and inputs)
SGMSE_KAT = torch.tensor([
    -0.8220521808+0.0136900125j, 0.6403278708-0.1466773599j, 0.0641574562-0.8893111944j,
    1.0807795525-0.0940670595j, -0.6070679426-0.2562257946j, 0.2370606065+0.0774136111j,
    0.6943444610-1.1398884058j, 0.3865116835-0.1694955975j, -0.3641569018-0.5190436840j,
    0.0308193229+0.7649886608j])


def sgmse_kat_inputs():
    def randn(*shape, dtype=torch.float32):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(0), dtype=dtype)

    def rand(*shape):
        return torch.rand(*shape, generator=torch.Generator().manual_seed(0))
    x = randn(4, 1, 256, 32, dtype=torch.cfloat)
    idx = torch.randint(x.numel(), (10,), generator=torch.Generator().manual_seed(0))
    return x, randn(4, 1, 256, 32, dtype=torch.cfloat), rand(4, 1, 1, 1), rand(4, 1, 1, 1), idx, randn


def test_sgmse_oracle_reproduces_the_reference_known_answer():
    """oracle/sgmse.py on the reference's own golden vector (default 65.6 M-parameter network,
    all weights 1e-3, batch of four noise levels)."""
    from brever_amd.models import SGMSEp, set_all_weights
    from oracle import sgmse as osg
    model = SGMSEp()
    with torch.no_grad():
        set_all_weights(model)
    x, y, sigma, t, idx, randn = sgmse_kat_inputs()
    model.model.net.emb.fourier_proj.b = randn(model.model.net.emb.fourier_proj.b.shape)
    net = osg.Net(model.state_dict(), 'model.net.', skip_scale=0.5**0.5)
    with torch.no_grad():
        out = osg.denoise(net, osg.RichterOUVE(), x, y, sigma, t)
    assert torch.allclose(out.flatten()[idx], SGMSE_KAT)


def test_dccrn_complex_batchnorm_oracle_matches_reference(golden_dir):
    """oracle ComplexBatchNorm2d variant of DCCRN vs the imported reference: train / eval
    outputs, running mean and covariance, loss and all gradients."""
    from oracle.criterion import snr
    from oracle.dccrn import OracleDCCRN
    g = np.load(os.path.join(golden_dir, 'dccrn.npz'))
    net = OracleDCCRN(**json.loads(str(g['cbn_config'])))
    _load_flat(net, g['cbn_params'])
    x = torch.from_numpy(g['x'])
    net.train()
    with torch.no_grad():
        y = net(x)
    assert torch.allclose(y, torch.from_numpy(g['cbn_out_train']), rtol=1e-4, atol=1e-6)
    running = torch.cat([b.reshape(-1).float() for n, b in net.named_buffers() if 'running' in n])
    assert torch.allclose(running, torch.from_numpy(g['cbn_running']), rtol=1e-5, atol=1e-7)
    batch, lengths = torch.from_numpy(g['batch']), torch.from_numpy(g['lengths'])
    loss = snr(net(batch[:, 0]), batch[:, 1], lengths).mean()
    assert abs(float(loss) - float(g['cbn_loss'])) <= 1e-5
    loss.backward()
    grads = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.allclose(grads, torch.from_numpy(g['cbn_grads']), rtol=2e-3, atol=1e-5)
    net.eval()
    with torch.no_grad():
        assert torch.allclose(net(x), torch.from_numpy(g['cbn_out_eval']), rtol=1e-4, atol=1e-6)


def test_causal_norm_oracle_matches_reference(golden_dir):
    """oracle.norm.causal_group_norm vs the reference's CausalLayerNorm / CausalGroupNorm /
    CausalInstanceNorm (frames last and on axis 2): outputs and the gradients wrt input, gain and
    bias, fp32, 1e-5 rel-L2."""
    from oracle.norm import causal_group_norm
    g = np.load(os.path.join(golden_dir, 'norms.npz'))
    x, gy = torch.from_numpy(g['x']), torch.from_numpy(g['gy'])
    for tag, groups, tdim in (('layer', 1, -1), ('group', 2, -1), ('instance', 6, -1), ('group_t2', 3, 2)):
        xg = x.clone().requires_grad_(True)
        gain = torch.from_numpy(g['gain']).requires_grad_(True)
        bias = torch.from_numpy(g['bias']).requires_grad_(True)
        y = causal_group_norm(xg, gain, bias, groups, tdim)
        (y*gy).sum().backward()
        for got, key in ((y.detach(), tag), (xg.grad, tag + '_dx'), (gain.grad, tag + '_dgain'),
                         (bias.grad, tag + '_dbias')):
            ref = torch.from_numpy(g[key])
            assert ((got - ref).norm()/ref.norm()).item() <= 1e-5, (tag, key)


def test_cumulative_norm_oracle_matches_reference(golden_dir):
    """oracle.norm.cumulative_norm in float64 vs the reference's CumulativeNormalizer output
    `cumnorm_out` of ffnn.npz. The golden is an fp32 cumsum and sits 1.4e-4 rel-L2 / 0.015 at the
    worst element from the float64 value (measured on the CPU): bounds 2e-4 / 0.02. On constant
    rows, where the reference's fp32 arithmetic is not finite, the oracle is finite and zero."""
    from oracle.norm import cumulative_norm
    g = np.load(os.path.join(golden_dir, 'ffnn.npz'))
    x, ref = torch.from_numpy(g['batch'])[:, :384].double(), torch.from_numpy(g['cumnorm_out']).double()
    y = cumulative_norm(x, 1e-4)
    assert y.dtype == torch.float64 and y.shape == ref.shape
    assert ((y - ref).norm()/ref.norm()).item() <= 2e-4
    assert (y - ref).abs().max().item() <= 0.02
    y2, mean, rstd = cumulative_norm(x, 1e-4, parts=True)
    assert torch.equal(y2, y) and (y - (x - mean)*rstd).abs().max().item() <= 1e-12
    for value in (-18.420681, -9.21, 0.0):
        const = torch.full((2, 3, 2000), value, dtype=torch.float32).double()
        yc = cumulative_norm(const, 1e-4)
        assert torch.isfinite(yc).all()
        assert yc.abs().max().item() <= 1e-9


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_tfgridnet_oracle_matches_reference(golden_dir, tag):
    """oracle.tfgridnet vs the reference TF-GridNet at seeded weights (two narrow configurations:
    one source / two sources with grid padding): output 1e-5, multiresyu loss 1e-5 relative, every
    parameter gradient 1e-4 (rel-L2 over the concatenation), fp32."""
    import json
    from oracle import tfgridnet as ot
    g = np.load(os.path.join(golden_dir, 'tfgridnet.npz'))
    cfg = json.loads(str(g[tag + '_config']))
    names = json.loads(str(g[tag + '_names']))
    flat = torch.from_numpy(g[tag + '_params'])
    shapes = ot.parameter_shapes(cfg)
    P, o = {}, 0
    for n in names:
        k = int(np.prod(shapes[n]))
        P[n] = flat[o:o + k].view(shapes[n]).clone().requires_grad_(True)
        o += k
    assert o == flat.numel()
    batch, lengths = torch.from_numpy(g[tag + '_batch']), torch.from_numpy(g[tag + '_lengths'])
    with torch.no_grad():
        out = ot.forward(P, cfg, batch[:, 0])
    ref = torch.from_numpy(g[tag + '_out'])
    assert ((out - ref).norm()/ref.norm()).item() <= 1e-5
    loss = ot.loss(P, cfg, batch, lengths)
    loss.backward()
    assert abs(loss.item() - float(g[tag + '_loss'])) <= 1e-5*abs(float(g[tag + '_loss']))
    grads = torch.cat([P[n].grad.reshape(-1) for n in names])
    gref = torch.from_numpy(g[tag + '_grads'])
    assert ((grads - gref).norm()/gref.norm()).item() <= 1e-4
