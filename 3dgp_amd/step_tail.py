"""The step tail on the device: what a training phase does after its backward passes, and the per-batch EMA update, in a constant number
of launches (csrc/step_tail.hip).

The eager tail (`training.optimizer_step`, `training.update_ema`) follows the reference (`training_loop.py:334-347`, `:357-367`): a
`torch.cat` of every gradient, `nan_to_num`, one `split` / `reshape` per tensor, `clip_grad_norm_`, a foreach Adam, and per batch a `lerp`
+ `copy_` per generator parameter and a `copy_` per buffer.  The number of launches grows with the number of tensors, not with the work.
Here a phase is four library launches whatever the number of tensors (pack; sanitise + per-block partial sums of squares; the reduction of
the partials; Adam with the clip coefficient read from device memory) and the EMA update is one.

Opt-in: `training.train_iteration(..., step_tail=True)` and `TrainingOptions.fused_step_tail`; `optimizer_step` and `update_ema` are
unchanged.

One difference from the eager tail, on purpose: after `FusedStepTail.step` the `p.grad` are views of the sanitised flat buffer, as after
`distributed.allreduce_gradients`, but they are NOT rescaled by the clip coefficient (`clip_grad_norm_` rescales them in place; here the
coefficient is applied inside the Adam kernel and the gradients stay as exchanged).  `record['norm']` is the device scalar the coefficient
was computed from.
"""
import numpy as np
import torch

from . import _lib

CHUNK = 4096                 # elements a block works on: TDGP_STEP_TAIL_CHUNK of include/tdgp.h (the library refuses another value)
ENTRY_LAUNCHES = dict(tdgp_grads_pack=1, tdgp_grads_sanitise_norm=2, tdgp_adam_step=1, tdgp_ema_update=1)     # kernel launches per call (include/tdgp.h)
_SLOTS = 4                   # pinned staging buffers for the per-step gradient-pointer table


def _chunk_map(counts):
    """chunk -> (tensor, first element) for tensors of `counts` elements each."""
    blocks = [-(-int(n) // CHUNK) for n in counts]
    tensor = np.repeat(np.arange(len(counts), dtype=np.int64), blocks)
    first = np.concatenate([np.arange(b, dtype=np.int64) * CHUNK for b in blocks]) if blocks else np.zeros(0, np.int64)
    return tensor, first


def _table(rows, counts, device):
    """Device table of include/tdgp.h: the rows, then the chunk map.  -> (tensor, num_blocks)"""
    tensor, first = _chunk_map(counts)
    words = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [tensor, first])
    return torch.from_numpy(words).to(device), int(tensor.size)


def _fits(t):
    return t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 4 == 0


class FusedStepTail:
    """`training.optimizer_step(module, opt, world, grad_clip)` for `torch.optim.Adam` (no amsgrad, no weight decay, no maximize, one
    parameter group) through the multi-tensor kernels.  The optimiser's own `exp_avg` / `exp_avg_sq` / `step` are used, so
    `opt.state_dict()` is what snapshots and resume expect and eager and fused steps may alternate on one optimiser."""

    def __init__(self, module, opt):
        if not isinstance(opt, torch.optim.Adam) or isinstance(opt, torch.optim.AdamW):
            raise NotImplementedError(f'FusedStepTail implements torch.optim.Adam, not {type(opt).__name__}')
        if len(opt.param_groups) != 1:
            raise NotImplementedError('FusedStepTail: one parameter group expected')
        g = opt.param_groups[0]
        if g.get('amsgrad') or g.get('weight_decay') or g.get('maximize') or g.get('capturable') or g.get('differentiable') or g.get('fused'):
            # (capturable / fused keep `step` on the device: reading it per tensor would synchronise once per tensor per step)
            raise NotImplementedError('FusedStepTail: amsgrad, weight decay, maximize, capturable, differentiable and fused=True are not built')
        self.module, self.opt = module, opt
        self.params = list(module.parameters())
        known = {id(p) for p in g['params']}
        if any(id(p) not in known for p in self.params):
            raise ValueError('FusedStepTail: a parameter of the module is not in the optimiser')
        self._plans = {}               # indices of the parameters that have a gradient -> (table, num_blocks, counts, offsets, total)
        self._stage, self._slot = None, 0
        self.record = None

    def _plan(self, key, params):
        """Device table for `params` (cached; rebuilt when a parameter or one of its state tensors has moved, e.g. after `load_state_dict`)."""
        state = [self.opt.state[p] for p in params]
        ptrs = tuple((p.data_ptr(), s['exp_avg'].data_ptr(), s['exp_avg_sq'].data_ptr()) for p, s in zip(params, state))
        plan = self._plans.get(key)
        if plan is not None and plan['ptrs'] == ptrs:
            return plan
        for p, s in zip(params, state):
            if isinstance(s['step'], torch.Tensor) and s['step'].is_cuda:
                raise RuntimeError('FusedStepTail: the optimiser keeps `step` on the device; the bias corrections are computed on the host')
            for t in (p, s['exp_avg'], s['exp_avg_sq']):
                if not (_fits(t) and t.is_cuda and t.numel() == p.numel()):
                    raise RuntimeError('FusedStepTail: parameters and optimiser state must be contiguous fp32 tensors on the GPU; there is no eager fall-back')
        counts = [p.numel() for p in params]
        offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        table, nb = _table([[q[0] for q in ptrs], [q[1] for q in ptrs], [q[2] for q in ptrs], counts, offsets], counts, params[0].device)
        plan = dict(ptrs=ptrs, table=table, num_blocks=nb, counts=counts, total=int(sum(counts)))
        self._plans[key] = plan
        return plan

    def _upload(self, words, device):
        """The per-step table through a small ring of pinned buffers (a slot is reused only after its copy has finished)."""
        n = len(words)
        if self._stage is None or self._stage[0][0].numel() < n:
            self._stage = [(torch.empty(max(n, 256), dtype=torch.int64).pin_memory(), torch.cuda.Event()) for _ in range(_SLOTS)]
            self._used = [False] * _SLOTS
        buf, ev = self._stage[self._slot]
        if self._used[self._slot]:
            ev.synchronize()
        buf[:n] = torch.as_tensor(words, dtype=torch.int64)
        out = buf[:n].to(device, non_blocking=True)
        ev.record()
        self._used[self._slot] = True
        self._slot = (self._slot + 1) % _SLOTS
        return out

    @torch.no_grad()
    def step(self, world=None, grad_clip=None):
        """-> record dict(launches, norm, flat, tensors).  `launches`: the kernel launches of the library calls this step made.  `norm` is a one-element fp64 DEVICE tensor (the 2-norm of the sanitised
        gradients); nothing is read back here."""
        idx = tuple(i for i, p in enumerate(self.params) if p.grad is not None)
        if not idx:
            self.record = dict(launches=0, norm=None, flat=None, tensors=0)
            return self.record
        params = [self.params[i] for i in idx]
        if any(p.numel() == 0 for p in params):
            raise RuntimeError('FusedStepTail: empty parameter')
        if world is None:
            import torch.distributed as dist
            world = dist.get_world_size() if dist.is_initialized() else 1
        group = self.opt.param_groups[0]
        for p in params:                                                    # torch.optim.Adam._init_group
            s = self.opt.state[p]
            if len(s) == 0:
                s['step'] = torch.tensor(0.0, dtype=torch.get_default_dtype())
                s['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                s['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        plan = self._plan(idx, params)
        device = params[0].device
        grads = []
        for p in params:
            g = p.grad
            if not (g.is_cuda and g.numel() == p.numel()):
                raise RuntimeError('FusedStepTail: gradients must reside on the GPU')
            grads.append(g if _fits(g) else g.float().contiguous())
        # the per-step table: gradient pointers, and per tensor -(lr / (1 - beta1^t)) and sqrt(1 - beta2^t) for ITS step count t, computed in
        # Python floats as torch does (tensors of one optimiser can be at different counts: a parameter without gradient in some phase)
        beta1, beta2 = (float(b) for b in group['betas'])
        lr, eps = float(group['lr']), float(group['eps'])
        ts = [float(self.opt.state[p]['step']) + 1 for p in params]
        factors = np.array([-(lr / (1.0 - beta1 ** t)) for t in ts] + [(1.0 - beta2 ** t) ** 0.5 for t in ts], dtype=np.float64)
        stab = self._upload(np.concatenate([np.array([g.data_ptr() for g in grads], dtype=np.int64), factors.view(np.int64)]), device)
        total, nb, T = plan['total'], plan['num_blocks'], len(params)
        flat = torch.empty(total, dtype=torch.float32, device=device)
        stream = _lib.stream_of(flat)
        made = []

        def call(name, *args):
            _lib.call(name, *args)
            made.append(name)
        call('tdgp_grads_pack', stab.data_ptr(), plan['table'].data_ptr(), T, nb, CHUNK, flat.data_ptr(), total, stream)
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(flat)
        nparts = -(-total // CHUNK)
        partials = torch.empty(nparts + 1, dtype=torch.float64, device=device)
        norm = partials[nparts:]
        call('tdgp_grads_sanitise_norm', flat.data_ptr(), total, int(world), CHUNK, partials.data_ptr(), nparts, norm.data_ptr(), stream)
        call('tdgp_adam_step', plan['table'].data_ptr(), stab.data_ptr(), T, nb, CHUNK, flat.data_ptr(), total, norm.data_ptr(),
                  -1.0 if grad_clip is None else float(grad_clip), beta1, beta2, eps, stream)
        # the kernels wrote through raw pointers: tell torch, so that everything keyed on `_version` (the packed-weight caches of ops/modconv.py
        # and generator.py, autograd's saved-tensor checks) sees the parameters as changed
        torch.autograd.graph.increment_version(params + [self.opt.state[p][k] for p in params for k in ('exp_avg', 'exp_avg_sq')])
        for p, g in zip(params, flat.split(plan['counts'])):
            self.opt.state[p]['step'] += 1
            p.grad = g.view(p.shape)
        self.record = dict(launches=sum(ENTRY_LAUNCHES[n] for n in made), norm=norm, flat=flat, tensors=T)       # counted from the calls made
        return self.record


def _ema_plan(G_ema, G):
    pairs = [(p, pe, 0) for pe, p in zip(G_ema.parameters(), G.parameters())] + [(b, be, 1) for be, b in zip(G_ema.buffers(), G.buffers())]
    fused, eager = [], []
    for s, d, kind in pairs:
        ok = _fits(s) and _fits(d) and s.is_cuda and d.is_cuda and s.shape == d.shape and s.numel() > 0
        (fused if ok else eager).append((s, d, kind))
    # the table is valid while the tensors it names stay where they are; the pairs on the eager path may move freely (the depth adaptor's
    # `progress_coef` gets new storage on every progressive_update)
    sig = tuple((s.data_ptr(), d.data_ptr(), s.numel()) for s, d, _ in fused)
    plan = G_ema.__dict__.get('_tdgp_ema_plan')              # lives and dies with G_ema
    if plan is None or plan['sig'] != sig:
        table, nb = None, 0
        if fused:
            counts = [s.numel() for s, _, _ in fused]
            table, nb = _table([[s.data_ptr() for s, _, _ in fused], [d.data_ptr() for _, d, _ in fused], counts, [k for _, _, k in fused]], counts,
                               fused[0][0].device)
        plan = G_ema.__dict__['_tdgp_ema_plan'] = dict(sig=sig, table=table, num_blocks=nb, tensors=len(fused))
    return dict(plan, eager=eager, written=[d for _, d, _ in fused])


@torch.no_grad()
def fused_update_ema(G_ema, G, cur_nimg, batch_size, ema_kimg=10.0, ema_rampup=0.05, ema_start_kimg=0.0):
    """`training.update_ema` in one launch: p_ema <- lerp(p, p_ema, beta) for every parameter pair and b_ema <- b for every buffer pair.
    beta == 0 copies bit for bit.  The table is cached on the device (parameter pointers are stable; it is rebuilt when one moves).  A pair
    that is not contiguous fp32 on the GPU takes the eager per-tensor ops, that pair only.  Returns beta, as `update_ema` does."""
    ema_nimg = ema_kimg * 1000
    if ema_rampup is not None:
        ema_nimg = min(ema_nimg, cur_nimg * ema_rampup)
    ema_beta = 0.5 ** (batch_size / max(ema_nimg, 1e-8))
    if ema_start_kimg > cur_nimg / 1000:
        ema_beta = 0.0
    plan = _ema_plan(G_ema, G)
    if plan['table'] is not None:
        _lib.call('tdgp_ema_update', plan['table'].data_ptr(), plan['tensors'], plan['num_blocks'], CHUNK, float(ema_beta), _lib.stream_of(plan['table']))
        torch.autograd.graph.increment_version(plan['written'])             # written through raw pointers: caches keyed on `_version` must see it
    for s, d, kind in plan['eager']:
        d.copy_(s if kind else s.lerp(d, ema_beta))
    return ema_beta
