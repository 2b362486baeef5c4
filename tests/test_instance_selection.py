"""Instance selection on the host: the closed form of 3dgp_amd/instance_selection.py (device=None) against scikit-learn's float64 run recorded in
tests/golden/instance_selection.npz (tools/gen_instance_selection_goldens.py), the top-k rule, the argument checks, and a folder filtered end to
end from stub embeddings.  No GPU here; the device route is tests/test_instance_selection_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('case1', 'case2')


@pytest.fixture(scope='module')
def S(tdgp):
    return tdgp.instance_selection


@pytest.fixture(scope='module')
def cases(golden):
    g = golden('instance_selection')
    return {c: {k[len(c) + 1:]: v for k, v in g.items() if k.startswith(c + '_')} for c in CASES}


def test_golden_is_what_the_tests_rely_on(cases):
    """Both sets cross a 64-column tile edge with n > 512; at every cut the float32 and float64 runs agree on the set and the gap is 10 x the noise."""
    assert cases['case1']['rows'].shape == (777, 130) and cases['case2']['rows'].shape == (600, 96)
    assert float(cases['case1']['reg_covar']) == 1e-5 and float(cases['case2']['reg_covar']) == 0.0
    for c in cases.values():
        assert c['rows'].dtype == np.float32 and c['scores64'].dtype == np.float64
        n = c['rows'].shape[0]
        assert list(c['cuts']) == [int(n * 0.5), int(n * 0.9)]
        noise = np.abs(c['scores32'] - c['scores64']).max()
        o32, o64 = np.argsort(c['scores32'], kind='stable'), np.argsort(c['scores64'], kind='stable')
        for k in c['cuts']:
            assert set(o32[n - k:]) == set(o64[n - k:])
            assert c['scores64'][o64[n - k]] - c['scores64'][o64[n - k - 1]] >= 10 * noise


@pytest.mark.parametrize('case', CASES)
def test_host_route_matches_the_float64_reference_run(S, cases, case):
    """device=None against scikit-learn's float64 run: within 1e-9 absolute (the raw-moment closed form sat at 2e-13 when the golden was made)."""
    c = cases[case]
    scores = S.compute_gaussian_ll_scores(c['rows'], reg_covar=float(c['reg_covar']), device=None)
    assert isinstance(scores, np.ndarray) and scores.dtype == np.float64 and scores.shape == (c['rows'].shape[0],)
    err = float(np.abs(scores - c['scores64']).max())
    print(f'{case}: host closed form vs the float64 reference run: {err:.3e}')
    assert err <= 1e-9
    n = len(scores)
    for k in c['cuts']:
        want = np.argsort(c['scores32'], kind='stable')[n - k:]                   # the reference's own (float32) selection
        assert set(S.select_instances(scores, int(k)).tolist()) == set(want.tolist())
    assert S.compute_gassian_ll_scores is S.compute_gaussian_ll_scores


def test_chunking_does_not_change_the_host_scores_beyond_rounding(S, cases, monkeypatch):
    c = cases['case2']
    whole = S.compute_gaussian_ll_scores(c['rows'], device=None)
    monkeypatch.setattr(S, 'CHUNK_ROWS', 97)
    parts = S.compute_gaussian_ll_scores(c['rows'], device=None)
    assert np.abs(whole - parts).max() <= 1e-9


def test_select_instances_order_and_ties(S):
    import torch
    scores = np.array([0.5, -1.0, 2.0, 0.5, 2.0, -3.0, 0.5])
    # ascending, stable: -3 (5), -1 (1), 0.5 (0, 3, 6), 2 (2, 4); of equal scores the later rows survive a cut through them
    assert S.select_instances(scores, 7).tolist() == [5, 1, 0, 3, 6, 2, 4]
    assert S.select_instances(scores, 4).tolist() == [3, 6, 2, 4]
    assert S.select_instances(scores, 1).tolist() == [4]
    got = S.select_instances(torch.from_numpy(scores), 4)
    assert isinstance(got, torch.Tensor) and got.tolist() == [3, 6, 2, 4]
    assert S.select_instances(scores, 3).tolist() == np.argsort(scores, kind='stable')[-3:].tolist()
    for bad in (0, 8, -1):
        with pytest.raises(ValueError, match='num_to_keep'):
            S.select_instances(scores, bad)


def test_scores_refuse_what_scikit_learn_refuses(S, cases):
    rows = cases['case2']['rows'].copy()
    bad = rows.copy()
    bad[17, 5] = np.nan
    with pytest.raises(ValueError, match='NaN or infinity'):
        S.compute_gaussian_ll_scores(bad, device=None)
    bad[17, 5] = np.inf
    with pytest.raises(ValueError, match='NaN or infinity'):
        S.compute_gaussian_ll_scores(bad, device=None)
    with pytest.raises(ValueError, match='reg_covar'):                              # n < F, no regularisation: a singular covariance
        S.compute_gaussian_ll_scores(rows[:50], reg_covar=0.0, device=None)
    dead = rows.copy()
    dead[:, 40] = 0.0                                                               # a dead feature: a zero pivot
    with pytest.raises(ValueError, match='reg_covar'):
        S.compute_gaussian_ll_scores(dead, reg_covar=0.0, device=None)
    assert np.isfinite(S.compute_gaussian_ll_scores(rows[:50], reg_covar=1e-5, device=None)).all()
    assert np.isfinite(S.compute_gaussian_ll_scores(dead, reg_covar=1e-5, device=None)).all()
    with pytest.raises(ValueError, match='N, F'):
        S.compute_gaussian_ll_scores(rows[0], device=None)
    with pytest.raises(ValueError, match='non-negative'):
        S.compute_gaussian_ll_scores(rows, reg_covar=-1.0, device=None)
    with pytest.raises(ValueError, match='GPU'):
        S.compute_gaussian_ll_scores(rows, device='cpu')


def _tree(root, names):
    from PIL import Image
    for i, name in enumerate(names):
        path = os.path.join(root, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if os.path.splitext(name)[1].lower() in ('.png', '.jpg'):
            Image.fromarray(np.full((4, 4, 3), i, np.uint8)).save(path)
        else:
            open(path, 'w').write('not an image')


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


NAMES = ['b/img3.png', 'a/img1.png', 'a/img0.PNG', 'a/notes.txt', 'b/img2.jpg', 'b/deep/img4.png', 'a/img5.png', 'b/img6.png', 'labels.json', 'a/img7.png']
# discovery order: a/img0.PNG a/img1.png a/img5.png a/img7.png b/deep/img4.png b/img2.jpg b/img3.png b/img6.png


def _stub_embeddings():
    """8 rows x 2 features, by discovery order: row 1 lies far out along the first feature, row 4 along the second."""
    return np.array([[0.1, 0.0], [5.0, 0.1], [-0.2, 0.3], [0.6, -0.4], [-0.3, -6.0], [0.0, 0.2], [1.0, 1.2], [-0.5, -1.8]], np.float32)


def test_argument_validation(S, tmp_path):
    src = str(tmp_path / 'src')
    _tree(src, NAMES)
    emb = _stub_embeddings()
    run = lambda **kw: S.run_instance_selection(src, str(tmp_path / 'out'), verbose=False, device=None, **kw)          # noqa: E731
    with pytest.raises(ValueError, match='Either num_imgs_to_keep or keep_ratio'):
        run(embeddings=emb)
    with pytest.raises(ValueError, match='Only one of'):
        run(embeddings=emb, num_imgs_to_keep=3, keep_ratio=0.5)
    with pytest.raises(ValueError, match='must be positive'):
        run(embeddings=emb, num_imgs_to_keep=0)
    for r in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match=r'keep_ratio must be in \(0, 1\]'):
            run(embeddings=emb, keep_ratio=r)
    with pytest.raises(ValueError, match='Exactly one of embeddings and detector'):
        run(num_imgs_to_keep=3)
    with pytest.raises(ValueError, match='Exactly one of embeddings and detector'):
        run(num_imgs_to_keep=3, embeddings=emb, detector=lambda x: x)
    with pytest.raises(ValueError, match=r'must be in \[1, 8\]'):
        run(embeddings=emb, num_imgs_to_keep=9)
    with pytest.raises(ValueError, match=r'must be in \[1, 8\]'):
        run(embeddings=emb, keep_ratio=0.1)                                        # int(8 * 0.1) = 0
    with pytest.raises(ValueError, match='7 rows'):
        run(embeddings=emb[:7], num_imgs_to_keep=3)
    assert not os.path.exists(tmp_path / 'out')


def test_folder_is_filtered_to_the_same_relative_paths(S, tmp_path):
    src, out = str(tmp_path / 'src'), str(tmp_path / 'out')
    _tree(src, NAMES)
    found = S.find_images_in_dir(src)
    assert found == [os.path.join(*p.split('/')) for p in
                     ['a/img0.PNG', 'a/img1.png', 'a/img5.png', 'a/img7.png', 'b/deep/img4.png', 'b/img2.jpg', 'b/img3.png', 'b/img6.png']]
    emb = _stub_embeddings()
    scores = S.compute_gaussian_ll_scores(emb, device=None)
    order = np.argsort(scores, kind='stable')
    kept = S.run_instance_selection(src, out, keep_ratio=0.7, embeddings=emb, verbose=False, device=None)      # int(8 * 0.7) = 5
    assert kept == [found[i] for i in order[-5:]]
    assert set(found) - set(kept) >= {found[1], found[4]}                           # the two outliers go
    assert _files(out) == sorted(kept)
    for p in kept:
        assert open(os.path.join(out, p), 'rb').read() == open(os.path.join(src, p), 'rb').read()


def test_subdir_wise_selects_inside_each_subdirectory(S, tmp_path):
    src, out = str(tmp_path / 'src'), str(tmp_path / 'out')
    _tree(src, NAMES)
    found = S.find_images_in_dir(src)
    emb = _stub_embeddings()
    kept = S.run_instance_selection(src, out, num_imgs_to_keep=3, subdir_wise=True, embeddings=emb, verbose=False, device=None)
    want = []
    for sub, rows in (('a', [0, 1, 2, 3]), ('b', [4, 5, 6, 7])):
        s = S.compute_gaussian_ll_scores(emb[rows], device=None)                    # each subdirectory has its own Gaussian
        want += [found[rows[i]] for i in np.argsort(s, kind='stable')[-3:]]
    assert kept == want and len(kept) == 6
    assert _files(out) == sorted(want)
    assert found[1] not in kept and found[4] not in kept
    # the whole folder at once keeps another set: 6 of 8 by one common Gaussian
    one = S.run_instance_selection(src, str(tmp_path / 'out1'), num_imgs_to_keep=6, embeddings=emb, verbose=False, device=None)
    assert len(one) == 6 and _files(str(tmp_path / 'out1')) == sorted(one)


def test_detector_route_feeds_uint8_batches_in_discovery_order(S, tmp_path):
    import torch
    src, out = str(tmp_path / 'src'), str(tmp_path / 'out')
    _tree(src, NAMES)
    emb = _stub_embeddings()
    seen = []

    def detector(images):
        assert images.dtype == torch.uint8 and images.ndim == 4 and images.shape[1:] == (3, 4, 4)
        seen.append(images[:, 0, 0, 0].tolist())
        return torch.from_numpy(emb[sum(len(s) for s in seen[:-1]):][:images.shape[0]])
    kept = S.run_instance_selection(src, out, num_imgs_to_keep=5, detector=detector, verbose=False, device=None)
    assert seen == [[2, 1, 6, 9, 5, 4, 0, 7]]                                       # the pixel value is the file's index in NAMES
    assert kept == S.run_instance_selection(src, str(tmp_path / 'out2'), num_imgs_to_keep=5, embeddings=emb, verbose=False, device=None)


def test_command_line_filters_a_folder_from_an_embeddings_file(S, tmp_path):
    """tools/run_instance_selection.py: the reference's flags plus --embeddings, one JSON line out (the host route here: no GPU in this test)."""
    src, out = str(tmp_path / 'src'), str(tmp_path / 'out')
    _tree(src, NAMES)
    np.save(tmp_path / 'emb.npy', _stub_embeddings())
    cmd = [sys.executable, os.path.join(REPO, 'tools', 'run_instance_selection.py'), '-s', src, '-o', out, '-n', '3', '--subdir_wise', '--reg_covar', '1e-05',
           '--embeddings', str(tmp_path / 'emb.npy'), '--device', 'cpu']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['num_images'] == 8 and res['num_kept'] == 6 and res['subdir_wise'] is True and res['device'] == 'cpu'
    assert _files(out) == sorted(res['kept'])
    assert res['kept'] == S.run_instance_selection(src, str(tmp_path / 'out2'), num_imgs_to_keep=3, subdir_wise=True, reg_covar=1e-5,
                                                   embeddings=_stub_embeddings(), verbose=False, device=None)
