"""The convolutions only training uses -- ops.conv2d_gradfix on csrc/conv_grad.hip (tdgp_conv2d, tdgp_conv2d_weight_grad) -- against
float64 at the tile edges of the two MFMA kernels, first and second order.

Reference everywhere: torch.nn.functional.conv2d on the CPU in float64 and autograd through it (a plain high-precision evaluation of
the same operation, independent of this repository's oracle).  Inputs are drawn from np.random.RandomState(cin * 131 + cout), cast to
fp32 and handed bit-identical to both sides.

Bars (the ones test_conv2d_strided / test_conv2d_gradfix_autograd / test_conv2d_weight_grad_oracle already hold these rows to):
  * y, dx, db and the second-order hx, hdy: 1e-5 of max|ref|;
  * dw and the second-order hw: 2e-5 of max|ref|.
The op is bilinear, so each second-order term is a single convolution of one of those kinds.  Next to every HIP figure the parity
report carries torch's own CPU fp32 run of the same graph against float64 (7e-8 .. 1.6e-6 on the ten cases: the bars leave ~10x).
"""
import warnings

import numpy as np
import pytest
import torch

from conftest import assert_close, max_rel, report_parity

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
OUT_TOL = 1e-5            # y, dx, db, hx, hdy (test_conv2d_strided)
WGRAD_TOL = 2e-5          # dw, hw (test_conv2d_weight_grad_oracle)
BARS = dict(y=OUT_TOL, dx=OUT_TOL, db=OUT_TOL, hx=OUT_TOL, hdy=OUT_TOL, dw=WGRAD_TOL, hw=WGRAD_TOL)

STRIDED, WGRAD, REDUCE, X2 = 'conv_strided_mfma_kernel', 'conv_wgrad_mfma_kernel', 'wgrad_reduce_kernel', 'z_gather_kernel'


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def N(t):
    return t.detach().float().cpu().numpy()


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()        # raises if libtdgp_hip.so is missing: GPU tests never run on a fallback


def _f64(t):
    return t.detach().double().cpu().numpy()


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


# ------------------------------------------------------------------------------------------------ 1. the forms, first and second order
# (B, Cin, Cout, H, W, k, stride, pad, bias), the branch of `_input_grad` dx takes, dx exactly 0 in the last row / column
FORM_CASES = [
    # D's down-conv form: odd input = 2 OH + 1 -> dx through _ConvTranspose2dX2.  OW = 66: two column tiles, the second 2 wide; three Cout blocks
    # with a 2-channel tail; 2.5 K chunks of 8 channels
    ((2, 20, 130, 9, 133, 3, 2, 0, True), 'x2', False),
    # Cin < 8: one ragged chunk; even sizes -> zero-stuffed dx; B = 3: the block index -> (b, oy) split
    ((3, 7, 12, 12, 16, 3, 2, 1, False), 'stuffed', False),
    # stride 1, pad 0; OW = 198: four column tiles, the last 6 wide; exact channel blocks
    ((1, 64, 64, 5, 200, 3, 1, 0, True), 'stuffed', False),
    # pad = k - 1; a Cout block holding one channel; a K chunk holding one channel
    ((2, 9, 65, 6, 70, 3, 1, 2, False), 'stuffed', False),
    # k = 1, stride 2 at width: OW = 70, 127 patch columns in use
    ((2, 33, 70, 10, 140, 1, 2, 0, True), 'stuffed', False),
    # stride 2 with pad 2
    ((1, 16, 8, 7, 9, 3, 2, 2, False), 'stuffed', False),
    # the last input row and column are never read: dx there is exactly 0 (the `H - LH + padding` completion of the zero-stuffed dy)
    ((1, 8, 8, 8, 130, 3, 2, 0, False), 'stuffed', True),
    # the native ('same') form for k = 3, 5, 1: modconv forward, same-conv dx; second order through the same _Conv2dGradWeight
    ((2, 20, 70, 12, 40, 3, 1, 1, True), 'same', False),
    ((1, 6, 10, 9, 11, 5, 1, 2, True), 'same', False),
    ((2, 24, 40, 11, 13, 1, 1, 0, False), 'same', False),
]


def _case_id(c):
    B, cin, cout, H, W, k, st, pad, bias = c[0]
    return f'{B}x{cin}x{H}x{W}-o{cout}-k{k}s{st}p{pad}' + ('-bias' if bias else '')


def _form_inputs(B, cin, cout, H, W, k, stride, pad, bias):
    rs = np.random.RandomState(cin * 131 + cout)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    t = dict(x=rs.randn(B, cin, H, W), w=rs.randn(cout, cin, k, k), b=rs.randn(cout) if bias else None, dy=rs.randn(B, cout, OH, OW),
             ex=rs.randn(B, cin, H, W), ew=rs.randn(cout, cin, k, k))
    return {n: None if v is None else torch.from_numpy(v.astype(np.float32)) for n, v in t.items()}


def _graph(conv, t, stride, pad):
    """y, the first-order gradients (kept differentiable) and the gradients of <dx, ex> + <dw, ew> w.r.t. x, w, dy."""
    x, w, dy = (t[n].detach().clone().requires_grad_(True) for n in ('x', 'w', 'dy'))
    b = None if t['b'] is None else t['b'].detach().clone().requires_grad_(True)
    y = conv(x, w, b, stride=stride, padding=pad)
    first = torch.autograd.grad(y, [x, w] + ([] if b is None else [b]), dy, create_graph=True)
    dx, dw = first[:2]
    hx, hw, hdy = torch.autograd.grad((dx * t['ex']).sum() + (dw * t['ew']).sum(), [x, w, dy])
    out = dict(y=y, dx=dx, dw=dw, hx=hx, hw=hw, hdy=hdy)
    if b is not None:
        out['db'] = first[2]
    return {n: v.detach() for n, v in out.items()}


def _cast(t, fn):
    return {n: None if v is None else fn(v) for n, v in t.items()}


@pytest.mark.parametrize('case', FORM_CASES, ids=_case_id)
def test_conv2d_forms_first_and_second_order(tdgp, case):
    """ops.conv2d_gradfix.conv2d on the GPU -- forward, dx / dw / db, and the three second-order terms R1 trains through -- against
    float64 at the smallest shapes that have a second column tile, a channel-block tail, a ragged K chunk, pad = k - 1, unread input
    edges, and each branch of `_input_grad`; the native kernels ran, repeats are bit-identical, a stride-0 dy equals its copy."""
    (B, cin, cout, H, W, k, stride, pad, bias), branch, zero_edge = case
    cg = tdgp.ops.conv2d_gradfix
    t = _form_inputs(B, cin, cout, H, W, k, stride, pad, bias)
    F = torch.nn.functional.conv2d
    ref = _cast(_graph(F, _cast(t, lambda v: v.double()), stride, pad), lambda v: v.numpy())
    ref32 = _cast(_graph(F, t, stride, pad), lambda v: v.numpy())
    tg = _cast(t, lambda v: v.to(DEV))
    assert all(torch.equal(tg[n].cpu(), t[n]) for n in t if t[n] is not None)

    got, names = _profiled(tdgp, lambda: _graph(cg.conv2d, tg, stride, pad))
    figs = {}
    for n in ref:
        figs['hip_' + n], figs['fp32_' + n] = max_rel(_f64(got[n]), ref[n], 1.0), max_rel(ref32[n], ref[n], 1.0)
    report_parity(f'conv2d training path {_case_id(case)} ({branch} dx)', kernels=','.join(sorted(names)),
                  worst_hip_over_fp32=max(figs['hip_' + n] / max(figs['fp32_' + n], 1e-30) for n in ref), **figs)

    # the native kernels ran (and nothing warned about a torch fallback: RuntimeWarning was an error)
    assert {WGRAD, REDUCE} <= names, names
    if branch == 'same':
        assert STRIDED not in names and X2 not in names and len(names) > 2, names
    else:
        assert STRIDED in names, names
        assert (X2 in names) == (branch == 'x2'), names

    assert set(got) == set(ref) and ('db' in ref) == bias
    for n in ref:
        assert got[n].dtype == torch.float32 and got[n].shape == ref[n].shape, n
        _check(n, _f64(got[n]), ref[n], BARS[n])
    if zero_edge:
        dx = got['dx']
        assert bool((dx[:, :, -1, :] == 0).all()) and bool((dx[:, :, :, -1] == 0).all()), 'dx of the unread last row / column is not exactly 0'
        assert not np.any(ref['dx'][:, :, -1, :]) and not np.any(ref['dx'][:, :, :, -1])

    # the sliced sums are deterministic by design: a second identical call is bit-identical
    again, _ = _profiled(tdgp, lambda: _graph(cg.conv2d, tg, stride, pad))
    for n in ('y', 'dx', 'dw'):
        assert torch.equal(got[n], again[n]), f'{n}: a second identical call differs'

    # dy as the stride-0 expanded tensor y.sum().backward() hands over: the same dx and dw as its contiguous copy
    def expanded():
        x, w = (tg[n].detach().clone().requires_grad_(True) for n in ('x', 'w'))
        y = cg.conv2d(x, w, tg['b'], stride=stride, padding=pad)
        y.sum().backward()
        dx1, dw1 = torch.autograd.grad(cg.conv2d(x, w, tg['b'], stride=stride, padding=pad), [x, w], torch.ones_like(y).contiguous())
        return x.grad, w.grad, dx1, dw1
    (dx0, dw0, dx1, dw1), _ = _profiled(tdgp, expanded)
    assert torch.equal(dx0, dx1) and torch.equal(dw0, dw1), 'stride-0 dy gives other gradients than its contiguous copy'
    ones = _cast(_graph(F, dict(_cast(t, lambda v: v.double()), dy=torch.ones_like(torch.from_numpy(ref['y']))), stride, pad), lambda v: v.numpy())
    _check('dx of y.sum()', _f64(dx0), ones['dx'], BARS['dx'])
    _check('dw of y.sum()', _f64(dw0), ones['dw'], BARS['dw'])


# ------------------------------------------------------------------------------------------------ 2. conv2d_weight_grad at the slice edges
def _wgrad_slices(B, cin, cout, OH, k):
    """csrc/conv_grad.hip:wgrad_slices -- the number of (b, oy)-row slices the weight gradient is summed in."""
    blocks_xy = -(-cout // 64) * -(-cin // 64) * k * k
    return max(1, min(-(-2048 // blocks_xy), B * OH, 256))


# (B, Cin, Cout, H, W, k, stride, pad), (slices, rows per slice, slices that hold rows)
WGRAD_EDGES = [
    # blocks_xy = 1 -> 2048 slices wanted, capped at 256; rows = 3 * 100 = 300 -> 2 rows per slice: slices 0 .. 149 hold the rows, 150 .. 255 are
    # empty and must contribute zeros (their partials are written, not skipped: the reduction reads all 256)
    ((3, 8, 8, 100, 5, 1, 1, 0), (256, 2, 150)),
    # rows = 257 -> 256 slices of 2 rows: slice 128 holds the single row 256, 129 .. 255 are empty.  OW = 33: every row has a second 32-pixel chunk
    # holding one pixel
    ((1, 5, 9, 257, 33, 1, 1, 0), (256, 2, 129)),
    # k = 7 (the largest the entry point admits) with pad 3: blocks_xy = 49 -> cdiv(2048, 49) = 42 slices wanted, rows = 10 -> 10 slices of one row
    ((1, 5, 6, 10, 12, 7, 1, 3), (10, 1, 10)),
    # the role-swapped stride-2 call of _ModulatedConv2dUp.backward at more than 64 channels on both sides: x := dz [2,70,17,19], dy := [2,130,8,9];
    # blocks_xy = 3 * 2 * 9 = 54 -> cdiv(2048, 54) = 38 slices wanted, rows = 2 * 8 = 16 -> 16 slices of one row
    ((2, 70, 130, 17, 19, 3, 2, 0), (16, 1, 16)),
]


@pytest.mark.parametrize('shape,slices', WGRAD_EDGES, ids=['empty_slices', 'one_row_slice_one_pixel_chunk', 'k7', 'role_swapped_s2'])
def test_conv2d_weight_grad_edges(tdgp, shape, slices):
    """conv2d_weight_grad directly, against the float64 dw, where `wgrad_slices` gets interesting: empty trailing slices (over a workspace
    that held NaNs), a last slice of one row, a second pixel chunk of one pixel, k = 7, the role-swapped stride-2 form of the x2 layers'
    backward with channel-block tails on both sides."""
    B, cin, cout, H, W, k, stride, pad = shape
    cg = tdgp.ops.conv2d_gradfix
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ns, per, used = slices
    rows = B * OH
    assert _wgrad_slices(B, cin, cout, OH, k) == ns and -(-rows // ns) == per and -(-rows // per) == used, 'the slice arithmetic stated in the table'
    nbytes = int(tdgp._lib.load().tdgp_conv2d_weight_grad_workspace_bytes(B, cin, cout, OH, k))
    assert nbytes == ns * cout * cin * k * k * 4, (nbytes, ns)

    rs = np.random.RandomState(cin * 131 + cout)
    x = torch.from_numpy(rs.randn(B, cin, H, W).astype(np.float32))
    dy = torch.from_numpy(rs.randn(B, cout, OH, OW).astype(np.float32))

    def dw_of(dtype):
        w0 = torch.zeros([cout, cin, k, k], dtype=dtype, requires_grad=True)
        return torch.autograd.grad(torch.nn.functional.conv2d(x.to(dtype), w0, None, stride=stride, padding=pad), [w0], dy.to(dtype))[0].numpy()
    ref, ref32 = dw_of(torch.float64), dw_of(torch.float32)

    xg, dyg = x.to(DEV), dy.to(DEV)
    junk = torch.full([nbytes // 4], float('nan'), device=DEV)       # the block the workspace is about to be carved from held NaNs
    del junk
    dw, names = _profiled(tdgp, lambda: cg.conv2d_weight_grad(xg, dyg, (cout, cin, k, k), stride, pad))
    report_parity(f'conv2d_weight_grad {"x".join(str(v) for v in shape)}: {ns} slices of {per} rows, {used} in use', kernels=','.join(sorted(names)),
                  hip_dw=max_rel(_f64(dw), ref, 1.0), fp32_dw=max_rel(ref32, ref, 1.0))
    assert names == {WGRAD, REDUCE}, names
    assert dw.shape == (cout, cin, k, k)
    _check('dw', _f64(dw), ref, WGRAD_TOL)
    assert torch.equal(dw, cg.conv2d_weight_grad(xg, dyg, (cout, cin, k, k), stride, pad))


# ------------------------------------------------------------------------------------------------ 3. forms outside both native sets
@pytest.mark.parametrize('form', [dict(stride=3, padding=1), dict(stride=1, padding=2, dilation=2)], ids=['stride3', 'dilation2'])
def test_conv2d_fallback_forms_warn_and_agree(tdgp, form):
    """k = 3 with stride 3 / with dilation 2 has no native form: conv2d says so once -- one RuntimeWarning per form, however often it is
    called -- and the torch.nn.functional path it takes still matches float64 (forward, dx, dw, db)."""
    cg = tdgp.ops.conv2d_gradfix
    B, cin, cout, H, W, k = 2, 6, 10, 13, 17, 3
    rs = np.random.RandomState(cin * 131 + cout)
    F = torch.nn.functional.conv2d
    x, w, b = (torch.from_numpy(rs.randn(*s).astype(np.float32)) for s in ([B, cin, H, W], [cout, cin, k, k], [cout]))
    y64 = F(x.double(), w.double(), b.double(), **form)
    dy = torch.from_numpy(rs.randn(*y64.shape).astype(np.float32))

    def run(conv, cast):
        xs, ws, bs = (cast(v).requires_grad_(True) for v in (x, w, b))
        y = conv(xs, ws, bs, **form)
        return [y.detach()] + list(torch.autograd.grad(y, [xs, ws, bs], cast(dy)))
    ref = [_f64(v) for v in run(F, lambda v: v.double())]
    ref32 = [_f64(v) for v in run(F, lambda v: v.clone())]

    seen = set(cg._fallback_seen)
    cg._fallback_seen.clear()               # whatever ran before this test: the form is new to the module again
    tdgp._lib.profile_enable(True)
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            got = run(cg.conv2d, lambda v: v.to(DEV))
            got2 = run(cg.conv2d, lambda v: v.to(DEV))
        torch.cuda.synchronize()
        names = set(tdgp._lib.profile_report())
    finally:
        tdgp._lib.profile_enable(False)
        cg._fallback_seen.update(seen)
    mine = [c for c in caught if issubclass(c.category, RuntimeWarning) and 'conv2d_gradfix.conv2d' in str(c.message)]
    assert len(mine) == 1, [str(c.message) for c in caught]
    assert 'no native gfx950 form' in str(mine[0].message)
    assert not names & {STRIDED, WGRAD}, names
    tag = ('y', 'dx', 'dw', 'db')
    report_parity(f'conv2d fallback form {form}', **{'torch_gpu_' + n: max_rel(_f64(g), r, 1.0) for n, g, r in zip(tag, got, ref)},
                  **{'fp32_' + n: max_rel(r32, r, 1.0) for n, r32, r in zip(tag, ref32, ref)})
    for n, g, g2, r in zip(tag, got, got2, ref):
        _check(n, _f64(g), r, BARS[n])
        _check(n + ' (second call)', _f64(g2), r, BARS[n])
