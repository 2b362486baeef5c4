"""The C-ABI library: builds for gfx950, loads without a GPU, exports every symbol include/tdgp.h declares,
and the product never reaches into oracle/ (no compute calls here)."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(tdgp_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_entry_points():
    syms = header_symbols()
    assert 'tdgp_bias_act' in syms and 'tdgp_upfirdn2d' in syms and 'tdgp_modconv2d' in syms and 'tdgp_triplane_field' in syms
    assert len(syms) >= 20


def test_library_builds_loads_and_exports(tdgp):
    lib_path = tdgp.build.build_native()
    assert os.path.exists(lib_path)
    lib = tdgp._lib.load()
    assert lib.tdgp_version() >= 100
    for s in header_symbols():
        assert hasattr(lib, s), f'{s} declared in include/tdgp.h but not exported'
    assert sorted(tdgp._lib.EXPORTS) == header_symbols()
    out = subprocess.run(['nm', '-D', '--defined-only', lib_path], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r' T (tdgp_\w+)', out)))
    assert exported == header_symbols()


def test_library_is_gfx950_only(tdgp):
    lib_path = tdgp.build.build_native()
    data = open(lib_path, 'rb').read()
    assert b'gfx950' in data
    for other in (b'gfx942', b'gfx90a', b'sm_80', b'sm_90'):
        assert other not in data


def test_ops_refuse_cpu_tensors_on_native_only_paths(tdgp):
    import torch
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match='GPU'):
        tdgp.ops.modconv.modulated_conv2d(x, torch.zeros(2, 3, 3, 3), torch.ones(1, 3), padding=1)
    with pytest.raises(RuntimeError, match='GPU'):
        tdgp.renderer.simple_tri_plane_renderer(torch.zeros(1, 24, 4, 4), torch.zeros(1, 5, 3), tdgp.renderer.TriPlaneMLP(8, 16))


def test_product_never_imports_the_oracle():
    bad = []
    for root, _, files in os.walk(os.path.join(REPO, '3dgp_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                src = open(os.path.join(root, f), errors='ignore').read()
                if re.search(r'^\s*(import|from)\s+oracle\b', src, flags=re.M) or 'tdgp_oracle' in src or 'orc_' in src:
                    bad.append(os.path.join(root, f))
    assert not bad, bad


def test_reference_api_surface(tdgp):
    """Same names / defaults as src.torch_utils.ops.{bias_act,upfirdn2d,conv2d_resample} and the renderer callables."""
    import inspect
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert sig(tdgp.ops.bias_act.bias_act) == ['x', 'b', 'dim', 'act', 'alpha', 'gain', 'clamp', 'impl']
    assert sig(tdgp.ops.upfirdn2d.upfirdn2d) == ['x', 'f', 'up', 'down', 'padding', 'flip_filter', 'gain', 'impl']
    assert sig(tdgp.ops.upfirdn2d.upsample2d) == ['x', 'f', 'up', 'padding', 'flip_filter', 'gain', 'impl']
    assert sig(tdgp.ops.upfirdn2d.setup_filter) == ['f', 'device', 'normalize', 'flip_filter', 'gain', 'separable']
    assert sig(tdgp.ops.conv2d_resample.conv2d_resample) == ['x', 'w', 'f', 'up', 'down', 'padding', 'groups', 'flip_weight', 'flip_filter']
    assert sig(tdgp.ops.modconv.modulated_conv2d) == ['x', 'weight', 'styles', 'noise', 'up', 'down', 'padding', 'resample_filter', 'demodulate',
                                                      'flip_weight', 'fused_modconv']
    assert sig(tdgp.renderer.sample_rays) == ['c2w', 'fov', 'resolution', 'patch_params', 'device']
    assert sig(tdgp.renderer.simple_tri_plane_renderer)[:4] == ['x', 'coords', 'mlp', 'scale']
    assert sig(tdgp.renderer.ImportanceRenderer.forward)[:6] == ['self', 'planes', 'decoder', 'ray_origins', 'ray_directions', 'rendering_options']
    assert sorted(tdgp.ops.bias_act.activation_funcs) == sorted(['linear', 'relu', 'lrelu', 'tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish'])
    assert [tdgp.ops.bias_act.activation_funcs[k].cuda_idx for k in ['linear', 'relu', 'lrelu', 'tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish']] == list(range(1, 10))


def test_ref_impl_paths_cpu(tdgp, oracle):
    """`impl='ref'` (API parity with the reference) against the oracle -- CPU tensors, plain PyTorch ops."""
    import numpy as np
    import torch
    rs = np.random.RandomState(0)
    x = rs.randn(2, 5, 9, 7).astype(np.float32)
    b = rs.randn(5).astype(np.float32)
    for act in tdgp.ops.bias_act.activation_funcs:
        y = tdgp.ops.bias_act.bias_act(torch.as_tensor(x), torch.as_tensor(b), act=act, impl='ref').numpy()
        assert np.abs(y - oracle.bias_act(x, b, act=act)).max() < 1e-5
    f = tdgp.ops.upfirdn2d.setup_filter([1, 3, 3, 1])
    y = tdgp.ops.upfirdn2d.upsample2d(torch.as_tensor(x), f, impl='ref').numpy()
    assert np.abs(y - oracle.upsample2d(x, f.numpy())).max() < 1e-5
    y = tdgp.ops.upfirdn2d.upfirdn2d(torch.as_tensor(x), f, up=[3, 2], down=[2, 1], padding=[2, 1, 0, 3], gain=1.5, impl='ref').numpy()
    assert np.abs(y - oracle.upfirdn2d(x, f.numpy(), up=[3, 2], down=[2, 1], padding=[2, 1, 0, 3], gain=1.5)).max() < 1e-5


def test_state_dict_layout_matches_reference_names(tdgp):
    cfg = tdgp.config.config_mid()
    G = tdgp.generator.Generator(cfg)
    res = G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=1), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    keys = set(G.state_dict())
    assert 'synthesis.tri_plane_decoder.b4.const' in keys and 'synthesis.tri_plane_decoder.b8.conv0.affine.weight' in keys
    assert 'synthesis.tri_plane_mlp.model.1.bias' in keys and 'mapping.w_avg' in keys and 'mapping.embed.weight' in keys


def test_walk2_isa_check_runs_in_the_build(tdgp):
    """the hand-issued tap loads of triplane_walk2_kernel rely on a property of the GENERATED code (3dgp_amd/isa_check.py).  The
    build runs the check whenever field.hip is recompiled and keeps the listing it checked; here the same check is re-run on that listing
    (produced now if a pre-built tree was copied without it), every instantiation must be present and clean."""
    import importlib
    build = importlib.import_module('3dgp_amd.build')
    asm = os.path.join(build.CSRC, 'build', 'field.s')
    if not os.path.exists(asm):
        subprocess.check_call([build._hipcc()] + build.FLAGS + ['-S', '--cuda-device-only', '-o', asm, os.path.join(build.CSRC, 'field.hip')], stderr=subprocess.DEVNULL)
    res = build.verify_field_isa(asm)
    assert len(res) >= 2 and all(not bad for _, bad in res.values())
    main = [k for k in res if 'ILi8ELi4ELb0E' in k]            # the C3 instantiation: feat 32, hid 64, no tap output
    assert main and res[main[0]][0]['tap_loads'] == 48 and res[main[0]][0]['compiler_vmcnt_waits'] == []
    # and the checker does catch a violation: an instruction reading a tap register right after its load
    isa = importlib.import_module('3dgp_amd.isa_check')
    lines = open(asm).read().splitlines()
    i0 = next(i for i, ln in enumerate(lines) if re.match(r'^_ZN\S*triplane_walk2_kernelILi8ELi4ELb0E\S*:', ln))
    i1 = next(j for j in range(i0, len(lines)) if lines[j].strip().startswith('.amdhsa_kernel'))
    body = lines[i0:i1]
    heads = [i for i, ln in enumerate(body) if 'Loop Header: Depth=1' in ln]
    k = next(i for i in range(heads[-1], len(body)) if body[i].strip().startswith('buffer_load_dwordx4'))
    dst = re.search(r'v\[(\d+):\d+\]', body[k]).group(1)
    body.insert(k + 1, f'\tv_add_f32_e32 v0, v{dst}, v{dst}')
    _, bad = isa.check_kernel(body, 8)
    assert bad and 'touches the destination' in bad[0][0]


def test_walk2_isa_check_knows_the_sgpr_hazard_and_scratch(tdgp):
    """A vector instruction that writes an SGPR needs 5 wait states before a vector-memory instruction reads it; the compiler cannot pad a load
    issued from an asm statement.  That is how the hid_dim 16 instantiations of triplane_walk2_kernel sent loads out with a stale plane base; the
    build refuses such a listing now, and one that spills to scratch (hand-counted waits assume the producer's memory instructions are its own)."""
    import importlib
    isa = importlib.import_module('3dgp_amd.isa_check')
    load = '\tbuffer_load_dwordx4 v[4:7], v1, s[4:7], s0 offen'
    for gap, caught in ((['\ts_waitcnt lgkmcnt(1)'], True), (['\ts_nop 1', '\tv_add_u32_e32 v9, v8, v8'], True), (['\ts_nop 3'], True), (['\ts_nop 4'], False),
                        (['\tv_mov_b32_e32 v2, v3'] * 5, False)):
        bad = isa.check_sgpr_hazard(['\tv_readfirstlane_b32 s0, v2'] + gap + [load])
        assert bool(bad) == caught, (gap, bad)
    assert not isa.check_sgpr_hazard(['\ts_add_i32 s0, s1, s2', load])                       # a scalar instruction wrote it: no hazard
    assert not isa.check_sgpr_hazard(['\tv_readfirstlane_b32 s9, v2', load])                 # another register
    assert isa.check_sgpr_hazard(['\tv_readlane_b32 s5, v255, 3', '.LBB0_1:', load])         # part of the descriptor; a label does not end the look-back
    assert isa.check_sgpr_hazard(['\tv_add_co_u32_e64 v1, s[0:1], v2, v3', load])            # a carry-out is a write of the pair
    assert not isa.check_sgpr_hazard(['\tv_add_u32_e32 v1, s0, v2', load])                   # a source is not
    for end in ('\ts_endpgm', '\ts_branch .LBB0_9'):                                         # control never falls out of these: not a predecessor
        assert not isa.check_sgpr_hazard(['\tv_readfirstlane_b32 s0, v2', end, '.LBB0_1:', load])
    assert isa.check_sgpr_hazard(['\tv_readfirstlane_b32 s0, v2', '\ts_cbranch_scc1 .LBB0_9', load])      # a conditional branch falls through
    build = importlib.import_module('3dgp_amd.build')
    asm = os.path.join(build.CSRC, 'build', 'field.s')
    if not os.path.exists(asm):
        subprocess.check_call([build._hipcc()] + build.FLAGS + ['-S', '--cuda-device-only', '-o', asm, os.path.join(build.CSRC, 'field.hip')], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    res = isa.check_walk2_asm(text)
    assert len(res) == 10 and all(s['scratch_bytes'] == 0 and not bad for s, bad in res.values())      # F 16 / 32 x hid 32 / 64 / 128 (F 16: 32 / 64), with and without taps
    assert not any('ELi1ELb' in k for k in res), 'hid_dim 16 is kept off the producer / consumer walk (csrc/field.hip: launch_field_t)'
    name = next(iter(res))
    spilled = re.sub(r'(\.amdhsa_kernel ' + re.escape(name) + r'\n(?:.*\n){0,8}?\s*\.amdhsa_private_segment_fixed_size) 0', r'\1 48', text, count=1)
    assert spilled != text and any('scratch' in why for why, _ in isa.check_walk2_asm(spilled)[name][1])


def test_wino4_isa_check_runs_in_the_build(tdgp):
    """conv3_wino4_kernel's LDS-direct loads are hand-issued (M0 written inside the asm statement, which hipcc will not let a clobber
    list name) and its pair-form K loop ends in a hand-counted `vmcnt(4)`.  isa_check.check_wino4_asm verifies on the generated code that M0 is
    written only by those statements, that the K loop holds nothing but the 8 expected LDS-direct issue sites (U before V) and that vmcnt(4) is
    its only vector-memory wait; the build runs it whenever modconv.hip is recompiled.  Here: re-run on the kept listing, then three injected
    violations must each be caught."""
    import importlib
    build = importlib.import_module('3dgp_amd.build')
    isa = importlib.import_module('3dgp_amd.isa_check')
    asm = os.path.join(build.CSRC, 'build', 'modconv.s')
    if not os.path.exists(asm):
        subprocess.check_call([build._hipcc()] + build.FLAGS + ['-S', '--cuda-device-only', '-o', asm, os.path.join(build.CSRC, 'modconv.hip')], stderr=subprocess.DEVNULL)
    res_all = build.verify_modconv_isa(asm)
    res = {k: v for k, v in res_all.items() if 'wino4f' not in k and 'torgb' not in k}
    # torgb_mfma_kernel<.., FAST> (round 6): hand-issued skip taps in batches of 4 under hand-counted waits
    rest = {k: v for k, v in res_all.items() if 'torgb' in k}
    assert len(rest) == 9 and all(not bad for _, bad in rest.values()), {k[-40:]: bad[:1] for k, (_, bad) in rest.items() if bad}       # 6 one-role instances + 3 of torgb_ws_kernel
    assert all(s_['tap_loads'] == 4 * s_['batches'] == 4 * s_['hand_waits'] for s_, _ in rest.values())
    assert sorted(s_['stages'] for s_, _ in rest.values()) == [1] * 6 + [2] * 3
    assert len(res) == 2 and all(not bad for _, bad in res.values())
    assert all(s['lds_direct_sites'] == 8 and s['mfma'] == 36 and s['m0_writes'] > 0 for s, _ in res.values())
    # conv3_wino4f_kernel (round 6): every vector-memory read of its item loop is hand-issued; no spill, nothing of the compiler's to wait for behind the K loop
    resf = {k: v for k, v in res_all.items() if 'wino4f' in k}
    assert len(resf) == 1 and all(not bad for _, bad in resf.values())
    sf = next(iter(resf.values()))[0]
    assert sf['mfma'] == 144 and sf['lds_direct_sites'] >= 40 and sf['atomics'] >= 2 and sf['stores_behind_loop'] >= 16, sf
    lines = open(asm).read().splitlines()
    i0 = next(i for i, ln in enumerate(lines) if re.match(r'^_ZN\S*conv3_wino4_kernelILb1ELb1E\S*:', ln))
    i1 = next(j for j in range(i0, len(lines)) if lines[j].strip().startswith('.amdhsa_kernel'))
    body = lines[i0:i1]
    w = next(i for i, ln in enumerate(body) if 's_waitcnt vmcnt(4)' in ln)
    for inject, needle in (('\tglobal_load_dword v0, v[2:3], off', 'other than an LDS-direct load'), ('\ts_movrels_b32 s0, s1 ; uses m0', None),
                           ('\tv_readlane_b32 s0, v1, m0', 'm0 is touched')):
        if needle is None:
            continue
        b2 = list(body)
        b2.insert(w + 8, inject)                                   # inside the K loop (its body follows the latch block in the listing)
        _, bad = isa.check_wino4_kernel(b2)
        assert bad and any(needle in why for why, _ in bad), (inject, bad[:2])
    b3 = [ln for i, ln in enumerate(body) if not (i > w and ' lds' in ln and i < w + 120)]      # drop the first LDS-direct sites of the loop
    _, bad = isa.check_wino4_kernel(b3)
    assert bad
    # the fused kernel: a spill reload, a compiler-side load behind the K loop, a touched atomic destination are each caught
    f0 = next(i for i, ln in enumerate(lines) if re.match(r'^_Z\S*conv3_wino4f_kernel\S*:', ln))
    f1 = next(j for j in range(f0, len(lines)) if lines[j].strip().startswith('.amdhsa_kernel'))
    fbody = lines[f0:f1]
    last_mfma = max(i for i, ln in enumerate(fbody) if 'v_mfma' in ln)
    first_store = next(i for i in range(last_mfma, len(fbody)) if 'global_store_dwordx4' in fbody[i])
    at = next(i for i, ln in enumerate(fbody) if re.search(r'global_atomic_add v\d+, v\d+, v\d+, s\[', ln) and 's_waitcnt vmcnt(0)' not in ''.join(fbody[i:i + 6]))
    dst = re.search(r'global_atomic_add (v\d+),', fbody[at]).group(1)
    for pos, inject, needle in ((first_store, '\tscratch_load_dword v1, off, off offset:4', 'scratch access'),
                                (first_store, '\tglobal_load_dword v1, v[2:3], off', 'behind the K loop'),
                                (first_store, '\ts_waitcnt vmcnt(2)', 'wait behind the K loop'),
                                (at + 1, f'\tv_mov_b32_e32 v1, {dst}', 'destination of a returning atomic')):
        b2 = list(fbody)
        b2.insert(pos, inject)
        _, bad = isa.check_wino4f_kernel(b2)
        assert bad and any(needle in why for why, _ in bad), (inject, bad[:2])
    # ToRGB: a compiler-side load between two hand-counted waits, and a copy of a tap register still in flight, are each caught
    t0 = next(i for i, ln in enumerate(lines) if re.match(r'^_ZN\S*torgb_mfma_kernelILi3ELb1ELb1ELb0E\S*:', ln))
    t1 = next(j for j in range(t0, len(lines)) if lines[j].strip().startswith('.amdhsa_kernel'))
    tbody = lines[t0:t1]
    w8 = [i for i, ln in enumerate(tbody) if ln.strip() == 's_waitcnt vmcnt(8)' and tbody[i - 1].strip().startswith(';;#ASMSTART')]
    hl = [i for i, ln in enumerate(tbody) if ln.strip().startswith('global_load_dwordx4') and tbody[i - 1].strip().startswith(';;#ASMSTART')]
    dst = re.search(r'global_load_dwordx4 v\[(\d+):', tbody[hl[8]]).group(1)
    for pos, inject, needle in ((w8[3] + 2, '\tglobal_load_dword v1, v[2:3], off', 'between the hand-counted waits'),
                                (hl[8] + 2, f'\tv_mov_b32_e32 v1, v{dst}', 'in flight')):
        b2 = list(tbody)
        b2.insert(pos, inject)
        _, bad = isa.check_torgb_kernel(b2, 3)
        assert bad and any(needle in why for why, _ in bad), (inject, bad[:2])
    # a listing without loop annotations is reported as unreadable, not as an IndexError
    with pytest.raises(isa.IsaListingError):
        isa.check_kernel(['_Zfoo:', '\ts_endpgm'], 8)


def test_device_fault_word_is_exported_and_quiet(tdgp):
    """include/tdgp.h tdgp_device_fault: readable without a GPU (no fault word can be allocated -> 0), never raises."""
    assert tdgp._lib.device_fault() == 0 and tdgp._lib.device_fault(clear=True) == 0


def test_modconv2d_path_query_agrees_with_the_bench_mirrors(tdgp):
    """tdgp_modconv2d_path answers from the launch plan tdgp_modconv2d itself reads (no GPU needed).  bench.py prices the layers with hand-written
    mirrors of the selection: on every stride-1 3x3 layer shape of C1-C5 at B = 1 .. 32 (plain layers, aligned tensors, arithmetic mode 0) the
    two must name the same kernel family, and on the x2 layer shapes tdgp_modconv2d_takes_folded_up2 must be the path query's answer for the
    folded form."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(REPO, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    lib = tdgp._lib.load()
    DIRECT, CONV3, WINO2, WINO4, WINO4F, WINO4_SPLITK, WINO4_FOLDED = 0, 1, 3, 4, 5, 6, 7        # tdgp_conv_path (include/tdgp.h)
    STYLES, NOISE, DEMODULATE, ALIGNED, LRELU = 1, 4, 8, 16, 32                                    # TDGP_PATHQ_*
    plain = STYLES | NOISE | DEMODULATE | ALIGNED | LRELU
    header = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    for name, val in (('DIRECT', DIRECT), ('CONV3', CONV3), ('WINO2', WINO2), ('WINO4', WINO4), ('WINO4F', WINO4F), ('WINO4_SPLITK', WINO4_SPLITK),
                      ('WINO4_FOLDED', WINO4_FOLDED)):
        assert re.search(rf'TDGP_PATH_{name} = {val}\b', header), name
    for name, val in (('STYLES', STYLES), ('NOISE', NOISE), ('DEMODULATE', DEMODULATE), ('ALIGNED', ALIGNED), ('LRELU', LRELU)):
        assert re.search(rf'TDGP_PATHQ_{name} = {val}\b', header), name
    prev = lib.tdgp_set_conv_arith(0)
    try:
        stride1, x2 = set(), set()
        for cfg in (getattr(tdgp.config, f'config_c{i}')() for i in range(1, 6)):
            for i, r in enumerate(cfg.block_resolutions):
                stride1.add((cfg.channels[r], r))
                if i > 0:
                    x2.add((cfg.channels[r // 2], cfg.channels[r], r // 2))
        assert len(stride1) >= 8 and len(x2) >= 7
        seen = set()
        for B in (1, 2, 4, 8, 16, 32):
            for c, r in sorted(stride1):
                path = lib.tdgp_modconv2d_path(B, c, c, r, r, 3, 1, 0, plain)
                if (B, c, r) == (32, 128, 512):
                    # the one shape of the sweep left out (C4's 512^2 x 128 layer at B = 32): 2^30 input elements, one more than a call takes
                    # ("tensor too large": activations are addressed through 4 GiB buffer descriptors), so the query answers TDGP_EINVAL like the
                    # call would; the mirrors know nothing of that bound (the generator runs such a batch in chunks)
                    assert path == -1 and B * c * r * r == 1 << 30
                    continue
                fused, w4, w2 = bench.winograd4_fused_takes(B, c, c, r), bench.winograd4_takes(B, c, c, r), bench.winograd_takes(B, c, c, r)
                want = (WINO4F,) if fused else ((WINO4, WINO4_SPLITK) if w4 else ((WINO2,) if w2 else (DIRECT, CONV3)))
                assert path in want, (B, c, r, path, want)
                seen.add(path)
            for cin, cout, h in sorted(x2):
                takes = lib.tdgp_modconv2d_takes_folded_up2(B, cin, 4 * cout, h, h)
                path = lib.tdgp_modconv2d_path(B, cin, 4 * cout, h, h, 3, 1, 2, plain)
                assert path in (WINO4_FOLDED, -2) and takes == int(path == WINO4_FOLDED), (B, cin, cout, h, takes, path)     # -2 = TDGP_EUNSUPPORTED: the call refuses the folded form
                seen.add(path)
        assert {CONV3, DIRECT, WINO4, WINO4F, WINO4_SPLITK, WINO4_FOLDED, -2} <= seen, seen
        # the facts of the call count: an unaligned tensor or another arithmetic mode leaves the Winograd kernels
        assert lib.tdgp_modconv2d_path(16, 64, 64, 512, 512, 3, 1, 0, plain) == WINO4F
        assert lib.tdgp_modconv2d_path(16, 64, 64, 512, 512, 3, 1, 0, plain & ~ALIGNED) == CONV3
        lib.tdgp_set_conv_arith(4)
        assert lib.tdgp_modconv2d_path(16, 64, 64, 512, 512, 3, 1, 0, plain) == WINO4
        lib.tdgp_set_conv_arith(2)
        assert lib.tdgp_modconv2d_path(16, 64, 64, 512, 512, 3, 1, 0, plain) == CONV3
        assert lib.tdgp_modconv2d_path(16, 64, 64, 512, 512, 7, 1, 0, plain) == -2 and lib.tdgp_modconv2d_path(0, 64, 64, 512, 512, 3, 1, 0, plain) == -1
    finally:
        lib.tdgp_set_conv_arith(prev)


def test_fold_up2_table_is_the_x2_layer(tdgp):
    """ops/modconv.fold_up2_table: the stride-2 transposed 3x3 convolution + 4x4 FIR of conv2d_resample.py:108-125 (flip_weight=False) as four
    3x3 'same' correlations of x, one per output parity -- against the op's own reference path (torch CPU ops, float64), image borders
    included, for the generator's symmetric filter and for an asymmetric one (the flip convention)."""
    import numpy as np
    import torch
    M, CR = tdgp.ops.modconv, tdgp.ops.conv2d_resample
    rs = np.random.RandomState(0)
    x = torch.tensor(rs.randn(2, 3, 7, 9))
    w = torch.tensor(rs.randn(4, 3, 3, 3))
    for f in (tdgp.ops.upfirdn2d.setup_filter([1, 3, 3, 1]), torch.tensor(rs.rand(4, 4), dtype=torch.float32)):
        ref = CR.conv2d_resample(x, w, f=f, up=2, padding=1, flip_weight=False)
        P = torch.tensor(M.fold_up2_table(f.numpy()))
        weff = torch.einsum('pqijab,ocab->opqcij', P, w).reshape(16, 3, 3, 3)
        ph = torch.nn.functional.conv2d(x, weff, padding=1)                                   # channel 4 o + 2 py + px
        got = ph.reshape(2, 4, 2, 2, 7, 9).permute(0, 1, 4, 2, 5, 3).reshape(2, 4, 14, 18)
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
