"""The fused step tail (3dgp_amd/step_tail.py over csrc/step_tail.hip): tdgp_grads_pack, tdgp_grads_sanitise_norm, tdgp_adam_step and
tdgp_ema_update against the eager tail as it stands (`training.optimizer_step` with torch.optim.Adam, `training.update_ema`).

The yardstick rule.  Both arms start a step from their OWN fp32 state; that step is restated in float64 on the CPU from that state and the
sanitised fp32 gradients (hyper-parameters as Python floats, norm and clip coefficient in float64).  e_eager = max |eager - float64|,
e_fused = max |fused - float64| per tensor and quantity; asserted: e_fused <= max(2 e_eager, one fp32 ulp of the largest magnitude in the
tensor) -- the ulp is the final rounding, which an arm that happens to be exact on a one-element tensor does not show.  Restating every step
from the arm's own state keeps the two trajectories' drift out of the comparison: each figure is the rounding of ONE step."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import report_parity

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()


@pytest.fixture(scope='module')
def ST(tdgp):
    return tdgp.step_tail


class ParamSet(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def contract_counts(chunk):
    return [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]


VIEW_COUNT, NOGRAD_COUNT = 37, 11
NOGRAD_AT = 4                                   # the parameter in the middle that never gets a gradient in the three steps


def make_set(chunk, seed=0):
    """The counts of the contract, one parameter without gradient in the middle, and one parameter that is a view one element (4 bytes)
    into a larger tensor, in front of the large ones."""
    g = torch.Generator().manual_seed(seed)
    counts = contract_counts(chunk)
    tensors = [torch.randn(n, generator=g).to(DEV) for n in counts]
    tensors.insert(NOGRAD_AT, torch.randn(NOGRAD_COUNT, generator=g).to(DEV))
    big = torch.randn(VIEW_COUNT + 8, generator=g).to(DEV)
    view = big[1:1 + VIEW_COUNT]
    assert view.data_ptr() % 16 == 4
    tensors.insert(6, view)
    return ParamSet(tensors)


def make_grads(module, chunk, step):
    """Gradients of one step (None for the parameter without one): normal values of mixed scale, NaN / +inf / -inf at a chunk's first and
    last element and in the ragged tails."""
    g = torch.Generator().manual_seed(100 + step)
    out = []
    bad = [float('nan'), float('inf'), float('-inf')]
    for i, p in enumerate(module.ps):
        if i == NOGRAD_AT:
            out.append(None)
            continue
        n = p.numel()
        x = torch.randn(n, generator=g) * (10.0 ** torch.randint(-3, 2, (n,), generator=g).float())
        if n == 5:
            x[4] = bad[step % 3]
        if n == chunk + 1:
            x[chunk] = bad[(step + 1) % 3]
        if n == 2 * chunk + 5:
            for k, j in enumerate([0, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, 2 * chunk + 4]):
                x[j] = bad[(k + step) % 3]
        out.append(x.to(DEV))
    return out


def adam64(p, m, v, g, t, lr, b1, b2, eps, coef):
    """torch.optim.Adam's update in float64 (numpy)."""
    g = g * coef
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return p, m, v


def ulp_of_max(a64):
    return float(np.spacing(np.float32(np.abs(a64).max())))


def n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def state_of(opt, p):
    s = opt.state[p]
    return (n64(s['exp_avg']), n64(s['exp_avg_sq']), float(s['step'])) if len(s) else (np.zeros(p.numel()), np.zeros(p.numel()), 0.0)


@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999)])
@pytest.mark.parametrize('clip', ['active', 'inactive'])
def test_tail_contract(tdgp, ST, betas, clip):
    chunk, lr, eps = ST.CHUNK, 2e-3, 1e-8
    fused_mod = make_set(chunk)
    eager_mod = copy.deepcopy(fused_mod)
    mods = dict(fused=fused_mod, eager=eager_mod)
    opts = {k: torch.optim.Adam(m.parameters(), lr=lr, betas=betas, eps=eps) for k, m in mods.items()}
    # the parameter without gradient gets optimiser state first: one plain Adam step on it (and on the first parameter, which is therefore one
    # step ahead of the others from here on: bias corrections are per tensor), the same in both arms
    for k, m in mods.items():
        m.ps[NOGRAD_AT].grad = torch.full_like(m.ps[NOGRAD_AT], 0.25)
        m.ps[0].grad = torch.full_like(m.ps[0], -0.5)
        opts[k].step()
        opts[k].zero_grad(set_to_none=True)
    quiet = fused_mod.ps[NOGRAD_AT]
    quiet_before = [quiet.detach().clone()] + [opts['fused'].state[quiet][k].clone() for k in ('exp_avg', 'exp_avg_sq', 'step')]
    tail = ST.FusedStepTail(fused_mod, opts['fused'])
    worst = {}
    for step in range(3):
        grads = make_grads(fused_mod, chunk, step)
        have = [g for g in grads if g is not None]
        clean = torch.nan_to_num(torch.cat(have), nan=0, posinf=1e5, neginf=-1e5)
        norm64 = float(np.sqrt((n64(clean) ** 2).sum()))
        max_norm = norm64 * 0.37 if clip == 'active' else norm64 * 3.0
        coef64 = min(1.0, max_norm / (norm64 + 1e-6))
        before = {k: [(n64(p), *state_of(opts[k], p)) for p in m.ps] for k, m in mods.items()}
        for k, m in mods.items():
            for p, g in zip(m.ps, grads):
                p.grad = None if g is None else g.clone()
        tdgp.training.optimizer_step(eager_mod, opts['eager'], world=1, grad_clip=max_norm)
        versions = [p._version for p in fused_mod.ps]
        rec = tail.step(world=1, grad_clip=max_norm)
        assert rec['launches'] == 4 and rec['tensors'] == len(have)
        # written through raw pointers, and torch is told: caches keyed on `_version` (packed weights) see a stepped parameter as changed
        assert all((p._version > v) == (g is not None) for p, v, g in zip(fused_mod.ps, versions, grads))
        # sanitised gradients: nan_to_num of the inputs, bit for bit, and p.grad are its views
        assert torch.equal(rec['flat'].view(torch.int32), clean.view(torch.int32))
        off = 0
        for p, g in zip(fused_mod.ps, grads):
            if g is None:
                assert p.grad is None
                continue
            assert p.grad.data_ptr() == rec['flat'].data_ptr() + 4 * off and torch.equal(p.grad, clean[off:off + p.numel()].view(p.shape))
            off += p.numel()
        # the norm: exact fp64 squares, so its fp32 value is within one fp32 ulp of the float64 norm's
        got = np.float32(rec['norm'].item())
        assert abs(float(got) - float(np.float32(norm64))) <= float(np.spacing(np.float32(norm64))), (got, norm64)
        off = 0
        for i, g in enumerate(grads):
            if g is None:
                continue
            n = g.numel()
            g64 = n64(clean[off:off + n])
            off += n
            res = {}
            for k, m in mods.items():
                p0, m0, v0, t0 = before[k][i]
                want = adam64(p0, m0, v0, g64, t0 + 1, lr, betas[0], betas[1], eps, coef64)
                st = opts[k].state[m.ps[i]]
                assert float(st['step']) == t0 + 1
                have_now = (n64(m.ps[i]), n64(st['exp_avg']), n64(st['exp_avg_sq']))
                res[k] = [float(np.abs(a - b).max()) for a, b in zip(have_now, want)]
                floors = [ulp_of_max(w) for w in want]
            for q, name in enumerate(('p', 'exp_avg', 'exp_avg_sq')):
                e_f, e_e = res['fused'][q], res['eager'][q]
                key = (name, n)
                if key not in worst or e_f / max(e_e, 1e-300) > worst[key][0] / max(worst[key][1], 1e-300):
                    worst[key] = (e_f, e_e, floors[q])
                print(f'step {step} tensor {i} n={n} {name}: fused {e_f:.3e} eager {e_e:.3e} ulp {floors[q]:.3e}')
                assert e_f <= max(2 * e_e, floors[q]), (step, i, n, name, e_f, e_e, floors[q])
    for (name, n), (e_f, e_e, fl) in sorted(worst.items()):
        if n in (1, chunk + 1, 2 * chunk + 5):
            report_parity(f'step tail betas={betas} clip {clip}: {name}, n={n}, one step vs float64', fused=e_f, eager=e_e, ulp_of_max=fl)
    # the parameter without gradient and its state: untouched, bit for bit
    now = [quiet.detach()] + [opts['fused'].state[quiet][k] for k in ('exp_avg', 'exp_avg_sq', 'step')]
    for a, b in zip(quiet_before, now):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert quiet.grad is None


def test_launches_do_not_grow_with_the_number_of_tensors(tdgp, ST):
    """Counted by the library itself: with per-kernel timing on, every launch the library makes is recorded (`_lib.profile_report`).  A step over
    10 tensors and one over 200 make the same launches -- pack 1, sanitise + norm 2, Adam 1 -- and `record['launches']` says what was counted."""
    small = make_set(ST.CHUNK)
    many = ParamSet([torch.randn(1 + (i * 7) % 50, device=DEV) for i in range(200)])
    seen = []
    for mod in (small, many):
        opt = torch.optim.Adam(mod.parameters(), lr=1e-3, betas=(0.0, 0.99))
        for p in mod.ps:
            p.grad = torch.randn_like(p)
        tail = ST.FusedStepTail(mod, opt)
        tdgp._lib.profile_enable(True)
        try:
            rec = tail.step(world=1, grad_clip=1.0)
            counted = {k: v['launches'] for k, v in tdgp._lib.profile_report().items()}
        finally:
            tdgp._lib.profile_enable(False)
        seen.append((rec['tensors'], rec['launches'], counted))
    assert seen[0][0] == 10 and seen[1][0] == 200
    assert seen[0][2] == seen[1][2] == dict(grads_pack_kernel=1, grads_sanitise_kernel=1, grads_norm_kernel=1, adam_step_kernel=1)
    assert seen[0][1] == seen[1][1] == sum(seen[0][2].values())


def test_optimisers_with_their_step_on_the_device_are_refused(ST):
    mod = ParamSet([torch.randn(5, device=DEV)])
    for kw in (dict(fused=True), dict(capturable=True)):
        with pytest.raises(NotImplementedError):
            ST.FusedStepTail(mod, torch.optim.Adam(mod.parameters(), lr=1e-3, **kw))


def test_alternates_with_the_eager_step_and_survives_load_state_dict(tdgp, ST):
    """The optimiser's own state tensors are used: an eager step, a fused step, a state dict round trip (new state tensors) and another
    fused step leave `step` at 3 and keep the state dict's layout."""
    mod = ParamSet([torch.randn(n, device=DEV) for n in (5, ST.CHUNK + 1)])
    opt = torch.optim.Adam(mod.parameters(), lr=1e-3, betas=(0.0, 0.99))
    tail = ST.FusedStepTail(mod, opt)
    for kind in ('eager', 'fused', 'reload', 'fused'):
        if kind == 'reload':
            opt.load_state_dict(copy.deepcopy(opt.state_dict()))
            continue
        for p in mod.ps:
            p.grad = torch.randn_like(p)
        tdgp.training.optimizer_step(mod, opt, world=1) if kind == 'eager' else tail.step(world=1)
    sd = opt.state_dict()
    assert sorted(sd['state'][0]) == ['exp_avg', 'exp_avg_sq', 'step'] and all(float(s['step']) == 3 for s in sd['state'].values())
    assert all(bool(torch.isfinite(p).all()) for p in mod.ps)


# ---------------------------------------------------------------------------------------------------------------------------- EMA
class Net(torch.nn.Module):
    def __init__(self, chunk, seed, bf16_buffer=True):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=g)) for n in contract_counts(chunk)])
        self.register_buffer('avg', torch.randn(7, generator=g))
        self.register_buffer('filt', torch.randn(chunk + 3, generator=g))
        if bf16_buffer:
            self.register_buffer('bf16_stat', torch.randn(9, generator=g).to(torch.bfloat16))


def test_ema_beta_zero_is_a_bitwise_copy_and_buffers_always_are(tdgp, ST):
    G, G_ema = Net(ST.CHUNK, 1).to(DEV), Net(ST.CHUNK, 2).to(DEV)
    with torch.no_grad():
        G.ps[3][0] = float('inf')                                       # p + 0 * (p_ema - p) would turn these into NaN; a copy does not
        G_ema.ps[4][0] = float('inf')
    kw = dict(cur_nimg=1000, batch_size=32, ema_kimg=10.0, ema_rampup=0.05, ema_start_kimg=5.0)
    beta = ST.fused_update_ema(G_ema, G, **kw)
    assert beta == 0.0 == tdgp.training.update_ema(copy.deepcopy(G_ema), G, **kw)
    for a, b in zip(list(G_ema.parameters()) + list(G_ema.buffers()), list(G.parameters()) + list(G.buffers())):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                                  b.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize('cur_nimg', [64, 4000, 10 ** 7])
def test_ema_ramp_up_beta_against_update_ema(tdgp, ST, cur_nimg):
    """beta below and above 0.5 (at::lerp's two branches) and near 1: the yardstick rule of this file against `training.update_ema`."""
    G, fused = Net(ST.CHUNK, 1).to(DEV), Net(ST.CHUNK, 2).to(DEV)
    eager = copy.deepcopy(fused)
    before = [n64(p) for p in fused.parameters()]
    kw = dict(cur_nimg=cur_nimg, batch_size=32, ema_kimg=10.0, ema_rampup=0.05)
    versions = [t._version for t in list(fused.parameters()) + list(fused.buffers())]
    beta = ST.fused_update_ema(fused, G, **kw)
    assert beta == tdgp.training.update_ema(eager, G, **kw) and 0.0 < beta < 1.0
    assert all(t._version > v for t, v in zip(list(fused.parameters()) + list(fused.buffers()), versions))
    for p, pe0, pf, pg in zip(G.parameters(), before, fused.parameters(), eager.parameters()):
        want = n64(p) + beta * (pe0 - n64(p))
        e_f, e_e = float(np.abs(n64(pf) - want).max()), float(np.abs(n64(pg) - want).max())
        print(f'ema beta={beta:.6f} n={p.numel()}: fused {e_f:.3e} eager {e_e:.3e} ulp {ulp_of_max(want):.3e}')
        assert e_f <= max(2 * e_e, ulp_of_max(want)), (p.numel(), e_f, e_e)
    for bf, bg, b in zip(fused.buffers(), eager.buffers(), G.buffers()):
        assert torch.equal(bf, b) and torch.equal(bg, b) and bf.dtype == b.dtype
    report_parity(f'EMA update, beta={beta:.6f}, n={2 * ST.CHUNK + 5}, vs float64', fused=e_f, eager=e_e, ulp_of_max=ulp_of_max(want))


def test_ema_table_follows_a_parameter_that_moved(ST):
    G, G_ema = Net(ST.CHUNK, 1, bf16_buffer=False).to(DEV), Net(ST.CHUNK, 2, bf16_buffer=False).to(DEV)
    ST.fused_update_ema(G_ema, G, cur_nimg=0, batch_size=8, ema_start_kimg=1.0)
    G.ps[2].data = torch.full((4,), 3.0, device=DEV)                   # new storage: the cached table must not be used
    ST.fused_update_ema(G_ema, G, cur_nimg=0, batch_size=8, ema_start_kimg=1.0)
    assert torch.equal(G_ema.ps[2].detach(), torch.full((4,), 3.0, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------------- two ranks
def test_two_ranks_share_one_gpu(tmp_path, ST):
    """Two fresh child processes (tests/step_tail_ranks.py), gloo, both on GPU 0, each under its own `timeout`: rank r holds gradients g_r;
    after .step(world=2) both hold bit-identical parameters, equal to ONE process stepping on (g_0 + g_1) / 2 (exact for two addends)."""
    import socket
    import step_tail_ranks as R
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    base = str(tmp_path / 'ranks')
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HIP_VISIBLE_DEVICES='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen(['timeout', '-k', '10', '240', sys.executable, os.path.join(REPO, 'tests', 'step_tail_ranks.py'), base],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f'rank {r}: {se[-3000:]}'
    got = [torch.load(f'{base}.rank{r}.pt') for r in range(2)]
    mod, opt = R.make(DEV)
    g0, g1 = R.grads(mod, 0), R.grads(mod, 1)
    for p, a, b in zip(mod.ps, g0, g1):
        p.grad = ((a + b) / 2).to(DEV)
    ST.FusedStepTail(mod, opt).step(world=1, grad_clip=R.CLIP)
    for i, p in enumerate(mod.ps):
        want = p.detach().cpu()
        assert torch.equal(got[0][i].view(torch.int32), got[1][i].view(torch.int32)), i
        assert torch.equal(got[0][i].view(torch.int32), want.view(torch.int32)), i
