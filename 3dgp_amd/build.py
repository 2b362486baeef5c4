"""Build libtdgp_hip.so (gfx950) in-tree with hipcc.  No JIT at import time, no hipify, no Triton.

The reference JIT-compiles its CUDA plugins on first use through torch.utils.cpp_extension
(src/torch_utils/custom_ops.py:59-155).  Here the library is built ahead of time by
`__graft_entry__.build()` (hipcc cross-compiles without a GPU) and travels with the tree.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(CSRC, 'libtdgp_hip.so')
SOURCES = ['core.hip', 'bias_act.hip', 'upfirdn2d.hip', 'modconv.hip', 'conv_grad.hip', 'camera_rays.hip', 'frames_grid.hip', 'field.hip', 'field_deep.hip', 'sampling.hip', 'render_grad.hip', 'render_fused.hip', 'geometry.hip', 'iso_surface.hip', 'mesh_raster.hip', 'mesh_components.hip', 'mesh_surface.hip', 'mesh_simplify.hip', 'mesh_decimate.hip', 'mesh_distance.hip', 'mesh_rays.hip', 'mesh_texture.hip', 'metrics.hip', 'pair_dist.hip', 'gaussian.hip', 'augment.hip', 'step_tail.hip', 'resample.hip']
HEADERS = ['common.h', 'device_scan.h', 'shade.h', 'mesh_bary.h', 'mesh_hit.h', 'quadric_solve.h', 'modconv_bf16.inc', 'modconv_wino.inc', 'modconv_wino4.inc', 'modconv_wino4f.inc', 'modconv_host.inc', 'field_body.inc', 'field_grad.inc', 'field_walk2.inc', 'mc_table.inc', os.path.join('..', '..', 'include', 'tdgp.h')]
# -ffp-contract=off: fp32 chains that decide integer rows must round like the reference's eager ops;
# fused multiply-adds are written explicitly (fmaf_) where wanted.
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC', '-fvisibility=hidden',
         '-Wno-unused-result']


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError('hipcc not found')


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _isa_check_module():
    sys.path.insert(0, HERE)
    try:
        import isa_check
    finally:
        sys.path.pop(0)
    return isa_check


def _verify_isa(asm_path, what, check_name):
    """Run one of isa_check's checkers over a listing; a violation fails the build (and removes the listing, so the next build checks
    again).  TDGP_SKIP_ISA_CHECK=1 turns violations AND parse failures into warnings (a toolchain whose listings the checker cannot read
    must not leave the user without a library); a listing the checker cannot parse is reported as that, not as a bare IndexError."""
    isa_check = _isa_check_module()
    skip = os.environ.get('TDGP_SKIP_ISA_CHECK', '0') not in ('', '0')
    try:
        res = getattr(isa_check, check_name)(open(asm_path).read())
        bad = [(k, why, ins) for k, (_, v) in res.items() for why, ins in v]
        msg = None
        if not res:
            msg = f'no {what} instantiation found in the listing'
        elif bad:
            msg = '; '.join(f'{k}: {why} | {ins}' for k, why, ins in bad[:8])
    except isa_check.IsaListingError as e:
        res, msg = {}, f'listing not understood: {e}'
    if msg:
        full = f'ISA check of {what} failed (3dgp_amd/isa_check.py): {msg}'
        if skip:
            import warnings
            warnings.warn(full + ' -- TDGP_SKIP_ISA_CHECK is set: continuing')
            return res
        os.remove(asm_path)
        raise RuntimeError(full + ' (TDGP_SKIP_ISA_CHECK=1 downgrades this to a warning)')
    return res


def verify_field_isa(asm_path):
    """isa_check.check_walk2_asm over the assembly of field.hip (hand-issued tap loads of triplane_walk2_kernel)."""
    return _verify_isa(asm_path, 'triplane_walk2_kernel', 'check_walk2_asm')


def verify_modconv_isa(asm_path):
    """isa_check.check_wino4_asm + check_wino4f_asm over the assembly of modconv.hip (hand-issued LDS-direct loads of conv3_wino4_kernel and conv3_wino4f_kernel)."""
    res = dict(_verify_isa(asm_path, 'conv3_wino4_kernel', 'check_wino4_asm'))
    res.update(_verify_isa(asm_path, 'conv3_wino4f_kernel', 'check_wino4f_asm'))
    res.update(_verify_isa(asm_path, 'torgb_mfma_kernel (FAST)', 'check_torgb_asm'))
    return res


def build_native(force=False, verbose=False):
    """Compile every HIP source for gfx950 and link libtdgp_hip.so.  Returns the library path."""
    hipcc = _hipcc()
    objdir = os.path.join(CSRC, 'build')
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace('.hip', '.o'))
        if force or _stale(o, [s] + hdrs):
            jobs.append((s, o))

    def compile_one(job):
        s, o = job
        cmd = [hipcc] + FLAGS + ['-c', s, '-o', o]
        if verbose:
            print(' '.join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'hipcc failed for {s}:\n{r.stderr}')
        return o

    # field.hip and modconv.hip carry hand-issued loads whose safety is a property of the generated code (isa_check.py): whenever one of
    # them is recompiled its assembly is produced next to the object and checked; a violation fails the build.
    checked = [('field.hip', 'field.s', verify_field_isa), ('modconv.hip', 'modconv.s', verify_modconv_isa)]
    todo = []
    for src, lst, fn in checked:
        sp, ap = os.path.join(CSRC, src), os.path.join(objdir, lst)
        if any(s == sp for s, _ in jobs) or _stale(ap, [sp] + hdrs):
            todo.append((sp, ap, fn))

    def asm_one(item):
        sp, ap, _ = item
        r = subprocess.run([hipcc] + FLAGS + ['-S', '--cuda-device-only', '-o', ap, sp], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'hipcc -S failed for {sp}:\n{r.stderr}')

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs) + len(todo)))) as ex:
        futs = [ex.submit(asm_one, it) for it in todo]
        list(ex.map(compile_one, jobs))
        for f in futs:
            f.result()
    for _, ap, fn in todo:
        fn(ap)
    objs = [os.path.join(objdir, s.replace('.hip', '.o')) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'link failed:\n{r.stderr}')
    return LIB


if __name__ == '__main__':
    print(build_native(force='--force' in sys.argv, verbose=True))
