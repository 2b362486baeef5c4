"""The reduced-precision (bf16) conv layers -- tdgp_modconv2d_bf16: conv3_bf16_kernel, upconv_bf16_kernel + the bf16-output forms of
fir_act_kernel, the bf16-input forms of torgb_mfma_kernel; tdgp_cast_f32_bf16 -- against tests/bf16_model.py, a float64 model with the KERNELS'
rounding points.  (tests/test_gpu_parity.py keeps the loose comparison with the oracle, which rounds at the REFERENCE's points.)

Pass condition of a layer case:
  * outputs whose bf16 bits differ from the model's <= 2 * count_seq + 8, count_seq = the outputs that differ between exact and sequential-fp32
    accumulation of the model itself (computed here on the CPU, from the reference alone): only the order of the fp32 additions separates a
    correct kernel from the model, and a blocked MFMA sum is no noisier than a left-to-right one (factor 2: small binomial counts; + 8: a zero
    count must not demand bit equality).  The smallest defect of interest -- one wrong row, column or 32-channel chunk -- moves >= 3 % of the outputs;
  * no output further than 2^-6 max|ref| from the model (two bf16 ulps at the top of the range): a lone O(1) error cannot hide in the count;
  * a second call gives the same bits (no atomics on this path).
ToRGB with a skip returns q + upsample2d(skip) in fp32, q the bf16-valued term: the kernel forms the skip term from four taps with three fused
multiply-adds and a multiplication and adds it to q -- five fp32 roundings, each <= 2^-24 of a partial result that |q| + sum |tap * skip| bounds.
An output counts as differing there when it is further than 2^-21 (|q| + sum |tap * skip|) from the model (eight such roundings; a bf16 step of q
is >= 2^-9 |q|), and the single-output bound is 2^-6 max|q|, the bf16-valued term's own scale.

Also here: the acceptance tests of the raw entry against their Python mirror (ops.modconv.bf16_kernel_takes), the x2 kernel's LDS budget (the one
refusal only the C side makes), the noise alignment error, the small images the stride-1 kernel must refuse (H < 8: its two-sample style stage
does not cover the block's 10-row window) on the widened fallback and on the fp32 entry, and the cast kernel bit for bit."""
import importlib

import numpy as np
import pytest
import torch

import bf16_model as M
from conftest import assert_close, report_parity

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BF16_MAX, BF16_MEAN = 1.5e-2, 2e-3          # test_gpu_parity.py: the oracle comparison's worst element / mean, of the tensor scale


@pytest.fixture(scope='module')
def native():
    tdgp = importlib.import_module('3dgp_amd')
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()
    return tdgp


def T(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def N(t):
    return t.detach().float().cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                              b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def check_against_model(what, got, ref, seq):
    """got / ref / seq: bf16-valued fp32 arrays (kernel, model, model with sequential fp32 accumulation)."""
    count_seq, _ = M.count_differing(seq, ref)
    mism, worst = M.count_differing(got, ref)
    max_err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / np.abs(ref).max())
    print(f'{what}: {mism} of {ref.size} outputs differ (count_seq {count_seq}), max |d| / max|ref| = {max_err:.3e}')
    report_parity('bf16 vs model ' + what, differing=mism, count_seq=count_seq, outputs=int(ref.size), max_err=max_err)
    assert mism <= 2 * count_seq + 8, f'{what}: {mism} outputs differ from the model (count_seq {count_seq}), largest {worst:.3e} of the scale'
    assert max_err <= M.MAX_ONE_OUTPUT, f'{what}: an output is {max_err:.3e} of the scale from the model'


# ------------------------------------------------------------------------------------------------ 3x3 layers
def run_conv(tdgp, c, up, noise, act, clamp):
    mc = tdgp.ops.modconv
    nz = None if noise == 'none' else T(c['noise_' + noise])
    return mc.modconv_forward(T(c['x']).to(torch.bfloat16), mc.PackedConv(T(c['w'])), T(c['s']), noise=nz, bias=T(c['bias']), up=up, demodulate=c['s'] is not None,
                              act=act, clamp=clamp, fir=mc.fir_host_array(M.FIR) if up == 2 else None, dcoef=T(c['dcoef']))


def conv_layer_case(tdgp, up, shape, noise, act, clamp, styled=True):
    B, cin, cout, H, W = shape
    assert tdgp.ops.modconv.bf16_kernel_takes(3, up, cin, cout, H, W), 'the case must run on the bf16 kernels, not on the widened fallback'
    c = M.conv_case(up, shape, styled)
    ref, seq = M.conv_expect(c, noise, act, clamp)
    y = run_conv(tdgp, c, up, noise, act, clamp)
    assert y.dtype == torch.bfloat16 and y.shape == (B, cout, H * up, W * up)
    check_against_model(f'3x3 up{up} {shape} noise {noise} {act} clamp {clamp}' + ('' if styled else ' no styles'), N(y), ref, seq)
    assert same_bits(y, run_conv(tdgp, c, up, noise, act, clamp)), 'a second call gave other bits'


@pytest.mark.parametrize('act,clamp', M.ACTS)
@pytest.mark.parametrize('noise', M.NOISES)
@pytest.mark.parametrize('shape', M.STRIDE1_SHAPES)
def test_stride1_vs_model(native, shape, noise, act, clamp):
    conv_layer_case(native, 1, shape, noise, act, clamp)


@pytest.mark.parametrize('shape', M.STRIDE1_SHAPES)
def test_stride1_no_styles_vs_model(native, shape):
    """styles=None with demodulate=False (the Conv2dLayer form): activations staged unscaled, no demodulation coefficient."""
    conv_layer_case(native, 1, shape, 'const', 'lrelu', 256.0, styled=False)


@pytest.mark.parametrize('act,clamp', M.ACTS)
@pytest.mark.parametrize('noise', M.NOISES)
@pytest.mark.parametrize('shape', M.UP2_SHAPES)
def test_up2_vs_model(native, shape, noise, act, clamp):
    conv_layer_case(native, 2, shape, noise, act, clamp)


# ------------------------------------------------------------------------------------------------ ToRGB
def planes_cl(a, feat):
    """NCHW [B,C,h,w] -> the channel-last plane tensor [B,C/feat,h,w,feat]."""
    B, C, h, w = a.shape
    return T(a).reshape(B, C // feat, feat, h, w).permute(0, 1, 3, 4, 2).contiguous()


def run_torgb(tdgp, c, feat, gain, clamp, skip):
    mc = tdgp.ops.modconv
    B, cout, H, W = c['acc_f64'].shape
    y = mc.modconv_forward(T(c['x']).to(torch.bfloat16), mc.PackedConv(T(c['w'])), T(c['s']), bias=T(c['bias']), demodulate=False, act='linear', gain=gain, clamp=clamp,
                           skip=planes_cl(c['prev'], feat) if skip else None, fir=mc.fir_host_array(M.FIR) if skip else None, out_layout=1, out_feat=feat)
    assert y.dtype == torch.float32 and y.shape == (B, cout // feat, H, W, feat)
    return y


@pytest.mark.parametrize('gain,clamp', M.TORGB_FORMS)
@pytest.mark.parametrize('skip', [False, True])
@pytest.mark.parametrize('shape', M.TORGB_SHAPES)
def test_torgb_vs_model(native, shape, skip, gain, clamp):
    B, cin, cout, feat, H, W = shape
    assert native.ops.modconv.bf16_kernel_takes(1, 1, cin, cout, H, W, out_layout=1, out_feat=feat, demodulate=False, has_skip=skip)
    c = M.torgb_case(shape)
    q_ref, q_seq = M.torgb_expect(c, gain, clamp)
    y = run_torgb(native, c, feat, gain, clamp, skip)
    got = y.permute(0, 1, 4, 2, 3).reshape(B, cout, H, W).cpu().numpy()
    what = f'torgb {shape} gain {gain} clamp {clamp}' + (' + skip' if skip else '')
    if not skip:
        check_against_model(what, got, q_ref, q_seq)
    else:
        ref = q_ref.astype(np.float64) + c['skip_up']
        err = np.abs(got.astype(np.float64) - ref)
        mism = int((err > 2.0 ** -21 * (np.abs(q_ref) + c['skip_abs_up'])).sum())
        count_seq, _ = M.count_differing(q_seq, q_ref)
        max_err = float(err.max() / np.abs(q_ref).max())
        print(f'{what}: {mism} of {ref.size} outputs differ (count_seq {count_seq}), max |d| / max|q| = {max_err:.3e}')
        report_parity('bf16 vs model ' + what, differing=mism, count_seq=count_seq, outputs=int(ref.size), max_err=max_err)
        assert mism <= 2 * count_seq + 8, f'{what}: {mism} outputs differ from the model (count_seq {count_seq})'
        assert max_err <= M.MAX_ONE_OUTPUT, f'{what}: an output is {max_err:.3e} of the scale from the model'
    assert same_bits(y, run_torgb(native, c, feat, gain, clamp, skip)), 'a second call gave other bits'


# ------------------------------------------------------------------------------------------------ the raw entry: acceptance and errors
SENTINEL = -21846          # 0xAAAA as int16


def raw_bf16(tdgp, B, cin, cout, H, W, k, up, layout=0, feat=0, skip=False, noise=None, nbs=0, seed=0, demodulate=None, act=None):
    """One call of tdgp_modconv2d_bf16 through _lib.call on fresh random tensors; y is prefilled with a sentinel.  -> (y as int16, error or None)."""
    L, mc = tdgp._lib, tdgp.ops.modconv
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g).to(DEV).to(torch.bfloat16)
    packed = mc.PackedConv(torch.randn(cout, cin, k, k, generator=g).to(DEV))
    s = (1 + 0.5 * torch.randn(B, cin, generator=g)).to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    rgb = layout == 1
    demodulate = (not rgb) if demodulate is None else demodulate
    act = ('linear' if rgb else 'lrelu') if act is None else act
    prev = torch.randn(B * cout * max(H // 2, 1) * max(W // 2, 1), generator=g).to(DEV) if skip else None
    y = torch.full([B * cout * H * up * W * up * 2], SENTINEL, dtype=torch.int16, device=DEV)          # room for an fp32 output
    ws_bytes = L.load().tdgp_modconv2d_workspace_bytes(B, cin, cout, H, W, k, up)
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.float32, device=DEV)
    fir = mc.fir_host_array(M.FIR) if (up == 2 or skip) else None
    err = None
    try:
        with torch.cuda.device(DEV):
            L.call('tdgp_modconv2d_bf16', x.data_ptr(), packed.buf.data_ptr(), s.data_ptr(), None, L.ptr(noise), nbs, bias.data_ptr(), fir, L.ptr(prev), y.data_ptr(),
                   B, cin, cout, H, W, k, up, int(demodulate), 3 if act == 'lrelu' else 1, 0.2 if act == 'lrelu' else 0.0, M.SQRT2 if act == 'lrelu' else 1.0, 256.0, layout, feat, ws.data_ptr(), ws_bytes,
                   L.stream_of(x))
    except RuntimeError as e:
        err = e
    torch.cuda.synchronize()
    return y, err


# (k, up, Cin, Cout, H, W, out_layout, out_feat, skip), B = 2 -- both sides of every condition of the acceptance tests
ACCEPT_TABLE = [
    (3, 1, 32, 16, 8, 32, 0, 0, False),          # stride 1: the smallest shape taken
    (3, 1, 48, 16, 8, 32, 0, 0, False),          # Cin % 32
    (3, 1, 2048, 8, 8, 32, 0, 0, False),         # Cin <= 2048 ...
    (3, 1, 2080, 8, 8, 32, 0, 0, False),         # ... and beyond
    (3, 1, 32, 16, 8, 48, 0, 0, False),          # W % 32
    (3, 1, 32, 16, 8, 64, 0, 0, False),
    (3, 1, 32, 16, 7, 32, 0, 0, False),          # H >= 8: 7, 4 and 2 are refused, 9 taken
    (3, 1, 32, 16, 4, 32, 0, 0, False),
    (3, 1, 64, 16, 2, 64, 0, 0, False),
    (3, 1, 32, 16, 9, 32, 0, 0, False),
    (5, 1, 32, 8, 8, 32, 0, 0, False),           # k
    (1, 1, 32, 8, 8, 32, 0, 0, False),           # 1x1 in the NCHW layout
    (3, 1, 32, 16, 8, 32, 1, 4, False),          # 3x3 in the plane layout
    (3, 2, 32, 16, 4, 4, 0, 0, False),           # x2: taken
    (3, 2, 32, 16, 3, 4, 0, 0, False),           # ... at any H
    (3, 2, 32, 16, 4, 5, 0, 0, False),           # W % 2
    (3, 2, 48, 16, 4, 4, 0, 0, False),           # Cin % 32
    (3, 2, 2080, 8, 4, 4, 0, 0, False),          # Cin <= 2048
    (3, 2, 32, 16, 4, 4, 1, 4, False),           # x2 in the plane layout
    (1, 2, 32, 16, 4, 4, 0, 0, False),           # 1x1 with up = 2
    (1, 1, 32, 48, 8, 8, 1, 16, False),          # ToRGB: taken
    (1, 1, 32, 96, 8, 8, 1, 32, True),           # Cout <= 96 ...
    (1, 1, 32, 128, 8, 8, 1, 32, False),         # ... and beyond
    (1, 1, 32, 48, 8, 8, 1, 0, False),           # out_feat: missing,
    (1, 1, 32, 48, 8, 8, 1, 6, False),           # not a multiple of 4,
    (1, 1, 32, 48, 8, 8, 1, 32, False),          # not a divisor of Cout
    (1, 1, 32, 24, 3, 6, 1, 8, False),           # (H W) % 4
    (1, 1, 32, 24, 2, 6, 1, 8, False),
    (1, 1, 32, 24, 4, 3, 1, 8, False),           # odd W: taken without a skip,
    (1, 1, 32, 24, 4, 3, 1, 8, True),            # refused with one
    (1, 1, 32, 24, 6, 10, 1, 8, True),
]


@pytest.mark.parametrize('case', ACCEPT_TABLE, ids=lambda c: 'k{}up{}_{}to{}_{}x{}_l{}f{}{}'.format(*c[:8], '_skip' if c[8] else ''))
def test_acceptance_mirror(native, case):
    """ops.modconv.bf16_kernel_takes == "the raw entry does not answer TDGP_EUNSUPPORTED", and a refused call has launched nothing."""
    k, up, cin, cout, H, W, layout, feat, skip = case
    rgb = layout == 1
    takes = native.ops.modconv.bf16_kernel_takes(k, up, cin, cout, H, W, out_layout=layout, out_feat=feat, demodulate=not rgb, has_noise=False,
                                                 act='linear' if rgb else 'lrelu', has_fir=up == 2 or skip, has_skip=skip)
    y, err = raw_bf16(native, 2, cin, cout, H, W, k, up, layout, feat, skip)
    assert err is None or isinstance(err, native._lib.Unsupported), err
    assert takes == (err is None), (case, takes, err)
    if err is not None:
        assert bool((y == SENTINEL).all()), 'a refused call wrote to y'
    else:
        out = 2 * cout * H * up * W * up * (2 if rgb else 1)
        assert bool((y[:out] != SENTINEL).any()) and bool((y[out:] == SENTINEL).all())


@pytest.mark.parametrize('kw', [dict(demodulate=True), dict(act='lrelu'), dict(has_noise=True)], ids=lambda kw: next(iter(kw)))
def test_acceptance_mirror_torgb_form(native, kw):
    """The ToRGB kernel has no demodulation, no noise and no activation: each is refused by the raw entry and by the mirror."""
    B, cin, cout, feat, H, W = 2, 32, 48, 16, 8, 8
    mirror = dict(out_layout=1, out_feat=feat, demodulate=False, has_noise=False, act='linear', has_fir=False, has_skip=False)
    assert native.ops.modconv.bf16_kernel_takes(1, 1, cin, cout, H, W, **mirror)
    assert not native.ops.modconv.bf16_kernel_takes(1, 1, cin, cout, H, W, **dict(mirror, **kw))
    raw = dict(kw)
    if raw.pop('has_noise', False):
        raw['noise'] = torch.zeros(H * W, device=DEV)
    y, err = raw_bf16(native, B, cin, cout, H, W, 1, 1, 1, feat, **raw)
    assert isinstance(err, native._lib.Unsupported), err
    assert bool((y == SENTINEL).all())


def test_up2_lds_budget_refusal(native, oracle):
    """The documented exception of the mirror: the x2 kernel keeps the styles of every sample a block touches in LDS, and at Cin = 2048, B = 4,
    4 x 4 that does not fit -- only the C side refuses (nothing launched), modconv_forward widens and runs the fp32 kernels."""
    B, cin, cout, H, W = 4, 2048, 8, 4, 4
    mc = native.ops.modconv
    assert mc.bf16_kernel_takes(3, 2, cin, cout, H, W)
    y, err = raw_bf16(native, B, cin, cout, H, W, 3, 2)
    assert isinstance(err, native._lib.Unsupported), err
    assert bool((y == SENTINEL).all())
    rs = np.random.RandomState(11)
    x = M.bf16(rs.randn(B, cin, H, W).astype(np.float32))
    w = rs.randn(cout, cin, 3, 3).astype(np.float32)
    s = (1.0 + 0.5 * rs.randn(B, cin)).astype(np.float32)
    bias = rs.randn(cout).astype(np.float32)
    ref = oracle.bias_act_bf16(oracle.modulated_conv2d(x, w, s, up=2, demodulate=True, resample_filter=M.FIR, prec='bf16'), bias, act='lrelu', clamp=256)
    got = mc.modconv_forward(T(x).to(torch.bfloat16), mc.PackedConv(T(w)), T(s), bias=T(bias), up=2, demodulate=True, act='lrelu', clamp=256, fir=mc.fir_host_array(M.FIR))
    assert got.dtype == torch.bfloat16 and got.shape == (B, cout, 2 * H, 2 * W)
    assert_bf16_close(N(got), ref, f'widened x2 layer {cin}->{cout} @{H}')


def test_noise_alignment_is_einval(native):
    """A noise pointer 4 bytes off 16-byte alignment: TDGP_EINVAL (include/tdgp.h), not a refusal the caller could widen around."""
    B, cin, cout, H, W = 2, 32, 16, 8, 32
    base = torch.zeros(H * W + 4, device=DEV)
    assert base.data_ptr() % 16 == 0
    y, err = raw_bf16(native, B, cin, cout, H, W, 3, 1, noise=base[1:], nbs=0)
    assert isinstance(err, RuntimeError) and not isinstance(err, native._lib.Unsupported), err
    assert '(-1)' in str(err) and '16-byte aligned' in str(err), err
    assert bool((y == SENTINEL).all())
    y, err = raw_bf16(native, B, cin, cout, H, W, 3, 1, noise=base[4:], nbs=0)
    assert err is None, err


# ------------------------------------------------------------------------------------------------ small images on the stride-1 form
def assert_bf16_close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref) / np.abs(ref).max()
    report_parity('bf16 ' + what, max_err=float(err.max()), mean_err=float(err.mean()))
    assert err.max() <= BF16_MAX and err.mean() <= BF16_MEAN, f'{what}: max {err.max():.3e}, mean {err.mean():.3e}'


SMALL_H = [(4, 32, 4, 32), (10, 32, 6, 32), (3, 64, 2, 64)]          # x shapes [B,Cin,H,W]: a block's 10 virtual rows reach a third sample's real rows


def small_h_inputs(shape, cout=64):
    B, cin, H, W = shape
    rs = np.random.RandomState(B * 100 + cin + H)
    return dict(x=M.bf16(rs.randn(B, cin, H, W).astype(np.float32)), w=rs.randn(cout, cin, 3, 3).astype(np.float32), s=(1.0 + 0.5 * rs.randn(B, cin)).astype(np.float32),
                bias=rs.randn(cout).astype(np.float32), noise=(0.3 * rs.randn(B, 1, H, W)).astype(np.float32))


@pytest.mark.parametrize('shape', SMALL_H)
def test_small_h_refused_and_widened(native, oracle, shape):
    """H < 8: the raw bf16 entry refuses (conv3_bf16_kernel stages two samples' styles; these windows hold three), modconv_forward takes the widened
    fp32 fallback and agrees with the oracle's bf16 path."""
    B, cin, H, W = shape
    mc = native.ops.modconv
    assert not mc.bf16_kernel_takes(3, 1, cin, 64, H, W)
    y, err = raw_bf16(native, B, cin, 64, H, W, 3, 1)
    assert isinstance(err, native._lib.Unsupported), err
    assert bool((y == SENTINEL).all())
    c = small_h_inputs(shape)
    ref = oracle.bias_act_bf16(oracle.modulated_conv2d(c['x'], c['w'], c['s'], noise=c['noise'], demodulate=True, prec='bf16'), c['bias'], act='lrelu', clamp=256)
    got = mc.modconv_forward(T(c['x']).to(torch.bfloat16), mc.PackedConv(T(c['w'])), T(c['s']), noise=T(c['noise']), bias=T(c['bias']), demodulate=True, act='lrelu', clamp=256)
    assert got.dtype == torch.bfloat16 and got.shape == (B, 64, H, W)
    assert_bf16_close(N(got), ref, f'widened layer {cin}->64 @{H}x{W}, B {B}')


@pytest.mark.parametrize('arith', [0, 2])
@pytest.mark.parametrize('shape', SMALL_H)
def test_small_h_fp32_entry(native, oracle, shape, arith):
    """The fp32 entry at the same shapes (its stride-1 kernels stage styles by another scheme) against the float64-accumulating oracle, at the
    tolerance of test_modconv_oracle; default arithmetic and direct sums only."""
    c = small_h_inputs(shape)
    ref = oracle.modulated_conv2d(c['x'], c['w'], c['s'], noise=c['noise'], demodulate=True)
    prev = native._lib.set_conv_arith(arith)
    try:
        y = native.ops.modconv.modulated_conv2d(T(c['x']), T(c['w']), T(c['s']), noise=T(c['noise']), padding=1, demodulate=True)
    finally:
        native._lib.set_conv_arith(prev)
    assert_close(N(y), ref, 1e-5, f'fp32 modconv {shape} arith {arith}', 1.0)


# ------------------------------------------------------------------------------------------------ the cast
SPECIAL_BITS = [0x00000000, 0x80000000,                     # +-0
                0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,          # exact ties: to the even neighbour below / above, both signs
                0x3F808001, 0x3F807FFF,                     # just beyond / short of a tie
                0x3FFFFFFF, 0x3FFF8000, 0xBFFFC000,         # up into the next binade
                0x7F7FFFFF, 0x7F7F8000, 0xFF7F8000, 0x7F7F7FFF,          # up into infinity (and the largest value that stays finite)
                0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000,          # subnormals, the tie that rounds to zero, the smallest normal
                0x7F800000, 0xFF800000,                     # +-inf
                0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x7FFFFFFF]          # NaNs: quiet, signalling, every mantissa bit


@pytest.mark.parametrize('n', [0, 1, 2, 3, 511, 512, 513, 1_000_003])
def test_cast_f32_bf16_bits(native, n):
    """tdgp_cast_f32_bf16 == torch's x.to(torch.bfloat16) on the CPU (round to nearest even), bit for bit; NaN stays NaN."""
    rs = np.random.RandomState(n)
    u = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)          # every exponent, subnormals, infinities and NaNs included
    sp = np.array(SPECIAL_BITS, np.uint32)
    for start in (0, max(n - len(sp), 0)):                  # the specials at the head and at the (odd) tail
        m = min(len(sp), n - start)
        u[start:start + m] = sp[len(sp) - m:] if start else sp[:m]
    x = torch.from_numpy(u.view(np.float32).copy())
    ref = x.to(torch.bfloat16)
    xd = x.to(DEV)
    y = torch.full([n + 8], SENTINEL, dtype=torch.int16, device=DEV)
    with torch.cuda.device(DEV):
        native._lib.call('tdgp_cast_f32_bf16', xd.data_ptr() if n else None, y.data_ptr() if n else None, n, native._lib.stream_of(y))
    torch.cuda.synchronize()
    assert bool((y[n:] == SENTINEL).all()), 'wrote past the end'
    got = y[:n].cpu().view(torch.bfloat16)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan])
    if n >= len(sp):
        assert int(nan.sum()) >= 5 and bool(torch.isinf(ref[~torch.isinf(x) & ~nan]).any())          # the inputs do hold NaNs and values that round into infinity
