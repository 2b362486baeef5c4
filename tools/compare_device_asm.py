"""Is the device code of a HIP source the same in two trees?  For a host-side refactor of a file that also holds kernels.

    python tools/compare_device_asm.py OLD.s NEW.s
    python tools/compare_device_asm.py --compile OLD_TREE NEW_TREE [source, default 3dgp_amd/csrc/modconv.hip]

The listings are what the build makes for its ISA check (`hipcc` + build.FLAGS + `-S --cuda-device-only`; `--compile` produces them).  Compared
per kernel symbol -- the order of the template instantiations in the file may move --: the set of `.amdhsa_kernel` symbols, the kernel
descriptor of each and the instruction text of each.  Basic-block labels (and the comments that cite them) carry the function's ordinal in the
file (`.LBB12_3`); the ordinal is dropped before comparing.  Exit status 0 = identical.  `--allow-added` accepts kernels that exist only in NEW
(a refactor that instantiates a shared body once more); a kernel that disappears or changes still fails."""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(text):
    """-> {symbol: lines from its label to the end of the function, kernel descriptor included} of every kernel of a device listing."""
    lines = text.split('\n')
    names = [ln.split()[1] for ln in lines if ln.strip().startswith('.amdhsa_kernel')]
    ordinal = re.compile(r'(BB|func_begin|func_end)\d+')        # `.LBB12_3:`, `; in Loop: Header=BB12_3`
    norm = lambda ln: ordinal.sub(r'\1', ln)                       # noqa: E731
    start = {ln.split(':')[0]: i for i, ln in enumerate(lines) if ln[:1] not in ('.', ' ', '\t', '') and ':' in ln}
    out = {}
    for n in names:
        i0 = start[n]
        i1 = next(j for j in range(i0, len(lines)) if lines[j].startswith('.Lfunc_end'))      # the descriptor lies in front of it
        out[n] = [norm(ln) for ln in lines[i0:i1]]
    return out


def compare(old_text, new_text, allow_added=False):
    old, new = kernels(old_text), kernels(new_text)
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if old[n] != new[n])
    for what, names in (('only in OLD', gone), ('only in NEW', added), ('text differs', differ)):
        for n in names:
            print(f'{what}: {n}')
    same = len(set(old) & set(new)) - len(differ)
    print(f'{len(old)} kernels in OLD, {len(new)} in NEW: {same} identical, {len(differ)} differ, {len(gone)} only in OLD, {len(added)} only in NEW; '
          f'{sum(len(b) for b in new.values())} lines of kernel text compared')
    return not (gone or differ or (added and not allow_added))


def listing(tree, source, out):
    sys.path.insert(0, os.path.join(REPO, '3dgp_amd'))
    import build
    subprocess.check_call([build._hipcc()] + build.FLAGS + ['-S', '--cuda-device-only', '-o', out, os.path.join(tree, source)])
    return open(out).read()


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--allow-added']
    allow_added = '--allow-added' in sys.argv[1:]
    if args and args[0] == '--compile':
        source = args[3] if len(args) > 3 else os.path.join('3dgp_amd', 'csrc', 'modconv.hip')
        with tempfile.TemporaryDirectory() as d:
            texts = [listing(args[i], source, os.path.join(d, f'{i}.s')) for i in (1, 2)]
    else:
        texts = [open(a).read() for a in args[:2]]
    sys.exit(0 if compare(*texts, allow_added=allow_added) else 1)
