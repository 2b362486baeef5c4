"""The generator's training-path modulated convolutions -- ops.modconv._ModulatedConv2dSame / _ModulatedConv2dUp, the two autograd nodes every
synthesis layer and every ToRGB runs through under `forward_autograd` -- against float64 on every kernel family `plan_modconv` can hand them.

Their backward has no kernel of its own: dx is the inference kernel called again on dy with the flipped, transposed weights (Cin and Cout
swapped, the demodulation coefficients in the styles slot, no styles at all for ToRGB), the x2 backward is the FIR adjoint feeding a stride-2
convolution and a role-swapped weight gradient, and ds / the demodulation terms of dw are eager tensor algebra around those calls.  The goldens
of test_modulated_conv2d_autograd / _up_autograd all have W % 32 != 0, i.e. the DIRECT path; here each case is the smallest shape found that
reaches one family, and the family is PINNED three ways: `tdgp_modconv2d_path` for the forward call, the same query for the dx call, and the
profiler's kernel names over forward + backward -- a moved dispatch threshold fails here instead of moving a case onto another kernel.

Reference: tests/modconv_reference.py (torch CPU float64, autograd; tied to the original implementation's goldens by test_modconv_reference.py).
Inputs from np.random.RandomState(cin * 131 + cout): x leaky-ReLU-shaped (non-zero mean, as the layers see it), s = 1 + 0.5 randn, dy = randn,
fp32, bit-identical on both sides.

Bars (test_modulated_conv2d_autograd's): y 1e-5 of max|ref|; dx, dw, ds 2e-5 of max|ref|.  Next to every HIP figure the parity report carries
torch's own CPU fp32 run of the same unfused graph against float64.

Measured on an MI355X (max|got - ref| / max|ref|, HIP / torch CPU fp32):
   #  form (B, Cin, Cout, H, W)          forward -> dx          y                  dx                 dw                 ds
   1  3x3  (3, 20, 130, 9, 12)          DIRECT -> DIRECT       4.2e-7 / 4.2e-7    1.9e-7 / 2.4e-7    2.0e-7 / 3.9e-7    1.8e-7 / 3.3e-7
   2  3x3  (2, 42, 72, 16, 32)          CONV3 -> CONV3         3.9e-7 / 3.7e-7    2.3e-7 / 2.5e-7    2.5e-7 / 1.8e-6    2.5e-7 / 4.5e-7
   3  3x3  (4, 64, 64, 128, 128)        WINO2 -> WINO2         3.6e-7 / 3.8e-7    3.3e-7 / 3.0e-7    6.8e-7 / 1.1e-6    2.4e-7 / 2.7e-7
   4  3x3  (32, 64, 64, 64, 64)         WINO4F -> WINO4F       2.4e-6 / 3.7e-7    2.0e-6 / 3.3e-7    6.9e-7 / 2.0e-6    1.0e-6 / 2.7e-7
   5  3x3  (16, 132, 512, 32, 32)       WINO4 -> WINO4_SPLITK  5.1e-6 / 3.2e-7    3.0e-6 / 3.1e-7    1.0e-6 / 1.8e-6    1.7e-6 / 2.6e-7
   6  3x3  (4, 512, 512, 32, 32)        SPLITK -> SPLITK       2.3e-6 / 3.3e-7    2.4e-6 / 2.7e-7    1.1e-6 / 2.8e-6    1.7e-6 / 2.7e-7
   7  1x1  (2, 64, 96, 32, 32)          CONV1 -> CONV1         2.8e-7 / 2.8e-7    2.0e-7 / 3.9e-7    2.5e-7 / 7.0e-7    1.1e-7 / 1.9e-7
   8  1x1  (2, 136, 96, 16, 24)         CONV1 -> CONV1         3.2e-7 / 3.1e-7    1.9e-7 / 4.1e-7    2.0e-7 / 4.7e-7    1.1e-7 / 2.0e-7
   9  x2   (3, 24, 40, 8, 8)            UP                     1.8e-7 / 2.3e-7    7.4e-7 / 3.8e-7    1.8e-7 / 3.7e-7    3.5e-7 / 2.0e-7
  10  x2   (1, 32, 48, 64, 64)          UP                     2.2e-7 / 3.5e-7    1.1e-6 / 2.9e-7    2.9e-7 / 6.2e-7    2.9e-7 / 2.3e-7
  11  x2   (8, 64, 256, 32, 32)         WINO4_FOLDED           2.2e-6 / 4.0e-7    1.7e-6 / 2.6e-7    4.0e-7 / 1.3e-6    9.3e-7 / 2.8e-7
The direct and F(2x2) kernels sit at torch's own fp32 figures; the F(4x4) families (Winograd's larger transform constants) at 5 - 16 x them, the
worst, y of case 5, at half its bar.  Zero / 1e-3 styles on case 2's shape: y and dx of the zero sample exactly 0, everything else 1.8e-7 .. 3.6e-7
per sample.  The three layers' `forward_autograd` outputs equal their fused `forward` bit for bit.
"""
import collections
import warnings

import numpy as np
import pytest
import torch

import modconv_reference as R
from conftest import assert_close, max_rel, report_parity

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
Y_TOL, GRAD_TOL = 1e-5, 2e-5
BARS = dict(y=Y_TOL, dx=GRAD_TOL, dw=GRAD_TOL, ds=GRAD_TOL)

# tdgp_conv_path / TDGP_PATHQ_* (include/tdgp.h; test_abi.py checks the numbers against the header)
DIRECT, CONV3, WINO2, WINO4, WINO4F, WINO4_SPLITK, WINO4_FOLDED, UP, CONV1 = 0, 1, 3, 4, 5, 6, 7, 8, 10
STYLES, DEMODULATE, ALIGNED = 1, 8, 16

MFMA, WINO, W4, W4IN, W4F, SPLITK = 'conv_mfma_kernel', 'conv_wino_kernel', 'conv_wino4_kernel', 'wino4_input_kernel', 'conv_wino4f_kernel', 'splitk_reduce_kernel'
UPW4, UPMFMA, FIRACT, FIR = 'upconv_wino4_kernel', 'upconv_mfma_kernel', 'fir_act_kernel', 'upfirdn2d_4x4'
STRIDED, WGRAD, WREDUCE = 'conv_strided_mfma_kernel', 'conv_wgrad_mfma_kernel', 'wgrad_reduce_kernel'
# every kernel of the library that convolves, filters or reduces on this path (packing, demodulation and casts are not family choices)
COMPUTE = {MFMA, WINO, W4, W4IN, W4F, SPLITK, UPW4, UPMFMA, FIRACT, FIR, STRIDED, WGRAD, WREDUCE, 'torgb_mfma_kernel', 'upfirdn2d_generic', 'z_gather_kernel',
           'conv_bf16_kernel', 'upconv_bf16_kernel'}
_WG = {WGRAD, WREDUCE}
_UPBWD = {FIR, STRIDED} | _WG

# form: 'c3' = 3x3 demodulated (SynthesisLayer, up 1), 'rgb' = 1x1 without demodulation (ToRGBLayer), 'up' = the x2 layer.
# fwd / dx: the family of the forward call and of the dx call (`up`: fwd = the folded F(4x4) form or the transposed conv + FIR; no modconv dx call).
# kernels: the COMPUTE kernels forward + backward must run, exactly -- except SPLITK where it is not listed: the direct kernels split K by their
# own block count at launch, which is no family choice.
Case = collections.namedtuple('Case', 'form B cin cout H W fwd dx kernels note')
CASES = [
    Case('c3', 3, 20, 130, 9, 12, DIRECT, DIRECT, {MFMA} | _WG, 'any width; three Cout blocks with a 2-channel tail, 2.5 K chunks'),
    Case('c3', 2, 42, 72, 16, 32, CONV3, CONV3, {MFMA} | _WG, 'Cin % 4 == 2, Cout tail; dx with Cin 72 -> Cout 42'),
    Case('c3', 4, 64, 64, 128, 128, WINO2, WINO2, {WINO} | _WG, 'F(2x2): 256 items'),
    Case('c3', 32, 64, 64, 64, 64, WINO4F, WINO4F, {W4F} | _WG, 'F(4x4), transform inside the GEMM kernel: 256 items'),
    Case('c3', 16, 132, 512, 32, 32, WINO4, WINO4_SPLITK, {W4IN, W4, SPLITK} | _WG, 'F(4x4) through V with 33 chunks; dx 512 -> 132 splits K'),
    Case('c3', 4, 512, 512, 32, 32, WINO4_SPLITK, WINO4_SPLITK, {W4IN, W4, SPLITK} | _WG, 'split-K F(4x4) both ways'),
    Case('rgb', 2, 64, 96, 32, 32, CONV1, CONV1, {MFMA} | _WG, '96-row tile forward; dx with styles=None'),
    Case('rgb', 2, 136, 96, 16, 24, CONV1, CONV1, {MFMA} | _WG, 'dx with Cout 136: 128-row tile and tail'),
    Case('up', 3, 24, 40, 8, 8, UP, None, {UPMFMA, FIRACT} | _UPBWD, 'FIR adjoint on the register-window kernel (17 x 17 out)'),
    Case('up', 1, 32, 48, 64, 64, UP, None, {UPMFMA, FIRACT} | _UPBWD, '128-wide FIR tiles; FIR adjoint on the LDS kernel (129 x 129 out)'),
    Case('up', 8, 64, 256, 32, 32, WINO4_FOLDED, None, {W4IN, UPW4} | _UPBWD, 'folded F(4x4) forward; backward on FIR adjoint, stride-2 conv, swapped wgrad'),
]
DY_FORM_CASES = [1, 3, 9]          # cases 2, 4 and 10 of the table (1-based)


def _case_id(c):
    return f'{c.form}-{c.B}x{c.cin}x{c.H}x{c.W}-o{c.cout}'


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    lib = tdgp._lib.load()        # raises if libtdgp_hip.so is missing: GPU tests never run on a fallback
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    prev = lib.tdgp_set_conv_arith(0)
    yield
    lib.tdgp_set_conv_arith(prev)
    torch.set_num_threads(threads)


def _check(what, got, ref, tol):
    """assert_close at floor 1.0, naming where the largest difference sits (which tile / channel block / chunk)."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    worst = tuple(int(i) for i in np.unravel_index(int(np.argmax(d)), d.shape)) if d.size else ()
    assert_close(got, ref, tol, f'{what} (largest difference at index {worst} of {d.shape})', 1.0)


def _profiled(tdgp, fn):
    """fn() with the library's per-kernel profiler on and RuntimeWarning an error (`_note_fallback` cannot pass silently) ->
    (result, set of the library kernels that ran)."""
    tdgp._lib.profile_enable(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            out = fn()
        torch.cuda.synchronize()
        names = set(tdgp._lib.profile_report())
    finally:
        tdgp._lib.profile_enable(False)
    return out, names


def _f64(t):
    return t.detach().double().cpu().numpy()


def _inputs(c):
    """fp32 CPU tensors x, w, s, dy of a case (k = 1 for 'rgb', else 3)."""
    rs = np.random.RandomState(c.cin * 131 + c.cout)
    k, up = (1 if c.form == 'rgb' else 3), (2 if c.form == 'up' else 1)
    x = rs.randn(c.B, c.cin, c.H, c.W)
    x = np.where(x < 0, 0.2 * x, x) * np.sqrt(2)                       # what a layer's input looks like: the lrelu output of the layer before
    t = dict(x=x, w=rs.randn(c.cout, c.cin, k, k), s=1 + 0.5 * rs.randn(c.B, c.cin), dy=rs.randn(c.B, c.cout, c.H * up, c.W * up))
    return {n: torch.from_numpy(v.astype(np.float32)) for n, v in t.items()}


def _to_dev(t):
    tg = {n: v.to(DEV) for n, v in t.items()}
    assert all(torch.equal(tg[n].cpu(), t[n]) for n in t)
    return tg


def _reference(c, t, dtype=torch.float64):
    return R.modconv_grads(t['x'], t['w'], t['s'], t['dy'], up=2 if c.form == 'up' else 1, demodulate=c.form != 'rgb', dtype=dtype)


def _forward(tdgp, c, x, w, s):
    mc = tdgp.ops.modconv
    if c.form == 'up':
        return mc.modulated_conv2d_up_autograd(x, w, s, tdgp.ops.upfirdn2d.setup_filter([1, 3, 3, 1]).to(DEV))
    return mc.modulated_conv2d_autograd(x, w, s, demodulate=c.form == 'c3')


def _hip(tdgp, c, tg, wrt='xws', dy=None, backward=None):
    """y and the gradients w.r.t. the inputs named in `wrt` (only those require grad) -> dict(y, dx, dw, ds); a gradient autograd did not
    produce is None.  `backward`: a function of y that runs the backward itself (y.sum().backward()); the gradients are then the .grad."""
    x, w, s = (tg[n].detach().clone().requires_grad_(n in wrt) for n in 'xws')
    ins = dict(x=x, w=w, s=s)
    y = _forward(tdgp, c, x, w, s)
    if backward is not None:
        backward(y)
        grads = [ins[n].grad for n in wrt]
    else:
        grads = torch.autograd.grad(y, [ins[n] for n in wrt], tg['dy'] if dy is None else dy, allow_unused=True)
    out = dict(y=y.detach(), dx=None, dw=None, ds=None)
    out.update({'d' + n: g for n, g in zip(wrt, grads)})
    return out


def _assert_paths(tdgp, c):
    """The host-side plan query names the family the table states, for the forward call and for the dx call of the backward."""
    lib = tdgp._lib.load()
    B, cin, cout, H, W = c.B, c.cin, c.cout, c.H, c.W
    if c.form == 'up':
        folded = c.fwd == WINO4_FOLDED
        assert lib.tdgp_modconv2d_path(B, cin, cout, H, W, 3, 2, 0, STYLES | DEMODULATE | ALIGNED) == UP
        assert lib.tdgp_modconv2d_takes_folded_up2(B, cin, 4 * cout, H, W) == int(folded)
        assert (cin >= 64 and H * W >= 512) or not folded, 'ops.modconv asks for the folded form from 64 channels and 512 pixels on'
        if folded:
            assert lib.tdgp_modconv2d_path(B, cin, 4 * cout, H, W, 3, 1, 2, STYLES | DEMODULATE | ALIGNED) == WINO4_FOLDED
        return
    k = 1 if c.form == 'rgb' else 3
    fwd = lib.tdgp_modconv2d_path(B, cin, cout, H, W, k, 1, 0, STYLES | ALIGNED | (DEMODULATE if c.form == 'c3' else 0))
    dx = lib.tdgp_modconv2d_path(B, cout, cin, H, W, k, 1, 0, ALIGNED | (STYLES if c.form == 'c3' else 0))
    assert (fwd, dx) == (c.fwd, c.dx), f'{_case_id(c)}: forward / dx family {(fwd, dx)}, the table says {(c.fwd, c.dx)}'


def _assert_kernels(c, names):
    ran = names & COMPUTE
    assert ran - {SPLITK} == c.kernels - {SPLITK} and (SPLITK in ran or SPLITK not in c.kernels), f'{_case_id(c)}: ran {sorted(ran)}, expected {sorted(c.kernels)}'


# ------------------------------------------------------------------------------------------------ 1. parity against float64, family pinned
@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_modconv_training_path_vs_float64(tdgp, c):
    """y, dx, dw, ds of the autograd node against float64, on the kernel family the table names (plan query for the forward and the dx call,
    profiler names over forward + backward; no fallback warning)."""
    _assert_paths(tdgp, c)
    t = _inputs(c)
    ref, ref32 = _reference(c, t), _reference(c, t, torch.float32)
    tg = _to_dev(t)
    got, names = _profiled(tdgp, lambda: _hip(tdgp, c, tg))
    figs = {}
    for n in ('y', 'dx', 'dw', 'ds'):
        figs['hip_' + n], figs['fp32_' + n] = max_rel(_f64(got[n]), ref[n], 1.0), max_rel(ref32[n], ref[n], 1.0)
    report_parity(f'modconv training path case {CASES.index(c) + 1} {_case_id(c)} ({c.note})', kernels=','.join(sorted(names & COMPUTE)), **figs)
    _assert_kernels(c, names)
    for n in ('y', 'dx', 'dw', 'ds'):
        assert got[n].dtype == torch.float32 and tuple(got[n].shape) == ref[n].shape, n
        _check(n, _f64(got[n]), ref[n], BARS[n])


def test_every_family_is_covered():
    """Between them the cases run every kernel of the training path's modulated convolutions."""
    ran = set().union(*(c.kernels for c in CASES))
    assert {MFMA, WINO, W4, W4IN, W4F, SPLITK, UPW4, UPMFMA, FIRACT, FIR, STRIDED, WGRAD, WREDUCE} <= ran
    assert {c.fwd for c in CASES} | {c.dx for c in CASES} >= {DIRECT, CONV3, WINO2, WINO4, WINO4F, WINO4_SPLITK, WINO4_FOLDED, UP, CONV1}
    # the FIR adjoint writes (2H + 1) x (2W + 1) planes: upfirdn2d's LDS-tiled kernel takes those of >= 16 x 64, the register-window kernel the
    # rest (csrc/upfirdn2d.hip; one profiler name for both) -- the x2 cases hold one of each
    lds = {2 * c.H + 1 >= 16 and 2 * c.W + 1 >= 64 for c in CASES if c.form == 'up'}
    assert lds == {False, True}


# ------------------------------------------------------------------------------------------------ 2. determinism, subsets of needs_input_grad
@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_modconv_training_path_repeats_and_subsets(tdgp, c):
    """The same call twice is bit-identical; gradients asked for x only, s only and w only are bit-equal to those of the full call; under
    conv2d_gradfix.no_weight_gradients() dw is not produced and dx, ds are unchanged."""
    cg = tdgp.ops.conv2d_gradfix
    tg = _to_dev(_inputs(c))
    full, names = _profiled(tdgp, lambda: _hip(tdgp, c, tg))
    _assert_kernels(c, names)
    again, _ = _profiled(tdgp, lambda: _hip(tdgp, c, tg))
    for n in ('y', 'dx', 'dw', 'ds'):
        assert torch.equal(full[n], again[n]), f'{n}: a second identical call differs'
    for one in 'xsw':
        sub, names = _profiled(tdgp, lambda: _hip(tdgp, c, tg, wrt=one))
        assert torch.equal(sub['y'], full['y']) and torch.equal(sub['d' + one], full['d' + one]), f'd{one} asked for alone differs from the full call'
        assert all(sub['d' + n] is None for n in 'xws' if n != one)
        assert (WGRAD in names) == (one == 'w'), (one, names)               # no weight gradient is computed to be thrown away
    with cg.no_weight_gradients():
        nw, names = _profiled(tdgp, lambda: _hip(tdgp, c, tg))
    assert not cg.weight_gradients_disabled
    assert nw['dw'] is None and WGRAD not in names, names
    assert torch.equal(nw['dx'], full['dx']) and torch.equal(nw['ds'], full['ds']), 'dx / ds change under no_weight_gradients()'


# ------------------------------------------------------------------------------------------------ 3. forms of dy
@pytest.mark.parametrize('c', [CASES[i] for i in DY_FORM_CASES], ids=_case_id)
def test_modconv_training_path_dy_forms(tdgp, c):
    """dy as the stride-0 expanded tensor y.sum().backward() hands over, and a channels-last dy: the same bits as their contiguous copies."""
    tg = _to_dev(_inputs(c))
    ones = torch.ones_like(tg['dy'])
    by_copy, _ = _profiled(tdgp, lambda: _hip(tdgp, c, tg, dy=ones))
    seen = []

    def sum_backward(y):
        y.register_hook(lambda g: seen.append(g.stride()))
        y.sum().backward()
    by_sum, _ = _profiled(tdgp, lambda: _hip(tdgp, c, tg, backward=sum_backward))
    assert seen == [(0, 0, 0, 0)], f'y.sum().backward() handed over a dy of strides {seen}: this test is about the stride-0 form'
    dy_cl = tg['dy'].contiguous(memory_format=torch.channels_last)
    assert not dy_cl.is_contiguous() and torch.equal(dy_cl, tg['dy'])
    by_cl, _ = _profiled(tdgp, lambda: _hip(tdgp, c, tg, dy=dy_cl))
    plain, _ = _profiled(tdgp, lambda: _hip(tdgp, c, tg))
    for n in ('dx', 'dw', 'ds'):
        assert torch.equal(by_sum[n], by_copy[n]), f'{n}: stride-0 dy gives other bits than its contiguous copy'
        assert torch.equal(by_cl[n], plain[n]), f'{n}: channels-last dy gives other bits than its contiguous copy'


# ------------------------------------------------------------------------------------------------ 4. an edge of the demodulation algebra
def test_modconv_training_path_zero_and_tiny_styles(tdgp):
    """Case 2's shape with the styles of sample 0 all zero (d = 1e4: y exactly 0, every gradient finite) and those of sample 1 scaled by 1e-3.
    y, dx and ds are measured per sample against that sample's own max|ref| (the d = 1e4 sample would otherwise set the scale for the other);
    dw, a sum over the samples to which sample 0 contributes exactly nothing, against its own.  Same bars."""
    c = CASES[1]
    assert c.B == 2
    t = _inputs(c)
    t['s'][0] = 0.0
    t['s'][1] *= 1e-3
    ref, ref32 = _reference(c, t), _reference(c, t, torch.float32)
    assert not ref['y'][0].any() and not ref['dx'][0].any() and ref['ds'][0].any() and ref['y'][1].any()
    tg = _to_dev(t)
    got, names = _profiled(tdgp, lambda: _hip(tdgp, c, tg))
    _assert_kernels(c, names)
    figs = {}
    for n in ('y', 'dx', 'ds'):
        for b in range(c.B):
            figs[f'hip_{n}{b}'], figs[f'fp32_{n}{b}'] = max_rel(_f64(got[n][b]), ref[n][b], 1.0), max_rel(ref32[n][b], ref[n][b], 1.0)
    figs['hip_dw'], figs['fp32_dw'] = max_rel(_f64(got['dw']), ref['dw'], 1.0), max_rel(ref32['dw'], ref['dw'], 1.0)
    report_parity(f'modconv training path {_case_id(c)}, styles of sample 0 zero, of sample 1 x 1e-3', **figs)
    for n in ('y', 'dx', 'dw', 'ds'):
        assert bool(torch.isfinite(got[n]).all()), f'{n} is not finite'
    assert bool((got['y'][0] == 0).all()), 'y of the sample with zero styles is not exactly 0'
    for n in ('y', 'dx', 'ds'):
        for b in range(c.B):
            _check(f'{n} of sample {b}', _f64(got[n][b]), ref[n][b], BARS[n])
    _check('dw', _f64(got['dw']), ref['dw'], BARS['dw'])


# ------------------------------------------------------------------------------------------------ 5. the layers: training graph == fused forward
LAYER_CASES = [(3, W4F), (10, UPW4), (6, MFMA)]          # case 4 and case 11 as SynthesisLayer, case 7 as ToRGBLayer; the kernel both forwards run
CLAMP = 1.5


def _fill(rs, p, scale=1.0, shift=0.0):
    with torch.no_grad():
        p.copy_(torch.from_numpy(np.asarray(shift + scale * rs.randn(*p.shape), np.float32)).to(p.device).reshape(p.shape))


@pytest.mark.parametrize('idx,kernel', LAYER_CASES, ids=[_case_id(CASES[i]) for i, _ in LAYER_CASES])
def test_layer_forward_autograd_equals_fused_forward(tdgp, idx, kernel):
    """SynthesisLayer / ToRGBLayer.forward_autograd (noise_mode='const', lrelu, bias, clamp as differentiable ops after the autograd node) against
    the same module's fused `forward` (noise, bias, activation and clamp in the kernel's epilogue) to 1e-5 of the output range: the training graph
    and the inference kernel are one layer at shapes where the convolution runs on the Winograd / 96-row kernels."""
    c = CASES[idx]
    gen = tdgp.generator
    w_dim, up = 32, (2 if c.form == 'up' else 1)
    rs = np.random.RandomState(c.cin * 131 + c.cout + 1)
    if c.form == 'rgb':
        layer = gen.ToRGBLayer(c.cin, c.cout, w_dim, conv_clamp=CLAMP).to(DEV)
    else:
        layer = gen.SynthesisLayer(c.cin, c.cout, w_dim, resolution=c.H * up, up=up, conv_clamp=CLAMP).to(DEV)
        _fill(rs, layer.noise_const)
        _fill(rs, layer.noise_strength, 0.0, 0.3)
    _fill(rs, layer.weight)
    _fill(rs, layer.bias, 0.5)
    _fill(rs, layer.affine.weight)
    x = _inputs(c)['x'].to(DEV)
    w = torch.from_numpy(rs.randn(c.B, w_dim).astype(np.float32)).to(DEV)
    kw = {} if c.form == 'rgb' else dict(noise_mode='const')

    def fused():
        with torch.no_grad():
            return layer(x, w, **kw)
    ref, names_fused = _profiled(tdgp, fused)
    got, names_auto = _profiled(tdgp, lambda: layer.forward_autograd(x.clone().requires_grad_(True), w, **kw))
    assert got.requires_grad and got.shape == ref.shape == (c.B, c.cout, c.H * up, c.W * up)
    assert kernel in names_fused and kernel in names_auto, (names_fused, names_auto)
    refn, gotn = _f64(ref), _f64(got)
    clamped = float((np.abs(refn) == CLAMP).mean())
    assert 0.0 < clamped < 0.5, f'the clamp binds on {clamped:.3f} of the outputs: it is meant to bind on some, not most'
    report_parity(f'layer forward_autograd vs fused forward {_case_id(c)}', range_err=max_rel(gotn, refn, 1.0), clamped_share=clamped)
    _check('forward_autograd vs fused forward', gotn, refn, 1e-5)
