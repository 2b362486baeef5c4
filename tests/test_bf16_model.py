"""tests/bf16_model.py is not nonsense, and its accumulation-noise yardstick, on the CPU.

1. The model (the KERNELS' rounding points: bf16(W), bf16(x s), d on the fp32 accumulator) against the oracle's bf16 path (the REFERENCE's points:
   per-sample weights bf16(W s d)) -- two correct evaluations of one layer, apart by rounding noise: inside the bf16 tolerance of test_gpu_parity.
2. For every case of tests/test_bf16_layers_gpu.py: `count_seq`, the outputs whose final bf16 bits differ between exact (float64) and sequential
   fp32 accumulation of the same model, and the largest such difference -- printed and written to the parity report.  The GPU test bounds the
   kernels' mismatches by 2 * count_seq + 8."""
import numpy as np
import pytest

import bf16_model as M
from conftest import report_parity

BF16_MAX, BF16_MEAN = 1.5e-2, 2e-3          # test_gpu_parity.py: worst element / mean, of the tensor scale


def _assert_bf16_close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref) / np.abs(ref).max()
    report_parity('bf16 model vs the oracle: ' + what, max_err=float(err.max()), mean_err=float(err.mean()))
    assert err.max() <= BF16_MAX and err.mean() <= BF16_MEAN, f'{what}: max {err.max():.3e}, mean {err.mean():.3e}'


def test_round_bf16_matches_oracle(oracle):
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.randn(4096).astype(np.float32) * np.float32(10.0) ** rs.randint(-20, 20, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895313892515355e38, np.inf, -np.inf], np.float32)])
    assert np.array_equal(M.bf16(x).view(np.uint32), oracle.round_bf16(x).view(np.uint32))
    assert M.bf16(np.float32(1.00390625)) == 1.0 and M.bf16(np.float32(1.01171875)) == np.float32(1.015625)          # ties to even, both directions


@pytest.mark.parametrize('up,shape,noise', [(1, (2, 32, 64, 8, 32), 'const'), (1, (3, 64, 40, 9, 32), 'per_sample'), (2, (2, 32, 64, 3, 64), 'const'),
                                            (2, (3, 32, 48, 7, 10), 'none')])
def test_model_vs_oracle_conv(oracle, up, shape, noise):
    c = M.conv_case(up, shape)
    nz = None if noise == 'none' else c['noise_' + noise]
    ref = oracle.bias_act_bf16(oracle.modulated_conv2d(c['x'], c['w'], c['s'], noise=nz, up=up, demodulate=True, resample_filter=M.FIR, prec='bf16'), c['bias'],
                               act='lrelu', clamp=256)
    got, _ = M.conv_expect(c, noise, 'lrelu', 256.0)
    _assert_bf16_close(got, ref, f'3x3 up{up} {shape} noise {noise}')


@pytest.mark.parametrize('shape', [(2, 32, 48, 16, 8, 8), (2, 200, 96, 32, 8, 12)])
def test_model_vs_oracle_torgb(oracle, shape):
    c = M.torgb_case(shape)
    ref = oracle.bias_act_bf16(oracle.modulated_conv2d(c['x'], c['w'], c['s'], demodulate=False, prec='bf16'), c['bias'], act='linear', clamp=256)
    got, _ = M.torgb_expect(c, 1.0, 256.0)
    _assert_bf16_close(got, ref, f'torgb {shape}')
    up = oracle.upsample2d(c['prev'], M.FIR)                                           # the skip image: fp32 on both sides
    assert np.abs(c['skip_up'] - up).max() <= 1e-6 * np.abs(up).max()
    _assert_bf16_close(got + c['skip_up'], ref + up, f'torgb {shape} + skip')


def _yardstick(what, pairs):
    """pairs: (variant, exact, sequential).  Prints and reports count_seq per variant; nothing here can fail but the sanity bounds."""
    worst_all = 0.0
    for variant, ref, seq in pairs:
        n, worst = M.count_differing(seq, ref)
        print(f'{what} {variant}: count_seq = {n} of {ref.size}, largest differing |d| / max|ref| = {worst:.3e}')
        report_parity(f'bf16 model yardstick {what} {variant}', count_seq=n, outputs=int(ref.size), worst_differing=worst)
        # sequential fp32 accumulation is itself a correct evaluation: it moves an output by one rounding step, never by more than the GPU bound
        assert worst <= M.MAX_ONE_OUTPUT and n <= 0.01 * ref.size, (what, variant, n, worst)
        worst_all = max(worst_all, worst)
    return worst_all


@pytest.mark.parametrize('shape', M.STRIDE1_SHAPES)
def test_yardstick_stride1(shape):
    c = M.conv_case(1, shape)
    pairs = [(f'noise {nz} {act} clamp {cl}',) + M.conv_expect(c, nz, act, cl) for nz in M.NOISES for act, cl in M.ACTS]
    c0 = M.conv_case(1, shape, styled=False)
    pairs.append(('no styles, no demodulation',) + M.conv_expect(c0, 'const', 'lrelu', 256.0))
    _yardstick(f'3x3 {shape}', pairs)


@pytest.mark.parametrize('shape', M.UP2_SHAPES)
def test_yardstick_up2(shape):
    c = M.conv_case(2, shape)
    _yardstick(f'3x3 x2 {shape}', [(f'noise {nz} {act} clamp {cl}',) + M.conv_expect(c, nz, act, cl) for nz in M.NOISES for act, cl in M.ACTS])


@pytest.mark.parametrize('shape', M.TORGB_SHAPES)
def test_yardstick_torgb(shape):
    c = M.torgb_case(shape)
    _yardstick(f'torgb {shape}', [(f'gain {g} clamp {cl}',) + M.torgb_expect(c, g, cl) for g, cl in M.TORGB_FORMS])
