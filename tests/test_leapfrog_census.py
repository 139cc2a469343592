"""Build census of the packed fp32 lifting bodies (no GPU needed): with the leapfrog step rotation a pair of terms costs 2 accumulate
FMAs + 2 rotation FMAs, so the tightest source loop of a kernel that has a lifting body holds at most 4 packed instructions per pair --
against 5 with the three-shear form it replaced (157 in k_skyvis_rec_f32pk<64, false>, 85 in k_skyvis_grad_f32pk<false>)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lifting_loops_take_two_fmas_per_step(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'prisim_amd', 'csrc', 'skyvis_kernels.hip')
    out = tmp_path / 'skyvis_kernels.s'
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I/opt/rocm/include', '-S', '--cuda-device-only', src,
                          '-o', str(out)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    text = out.read_text()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta as KM
    # kernel -> (pairs per source, accumulate FMAs per pair): HC = 32 pairs of V; the gradient kernel's 16-channel tiles, 4 sets
    want = {'k_skyvis_rec_f32pkILi64ELb0E': (32, 2), 'k_skyvis_grad_f32pkILb0E': (8, 8)}
    seen = set()
    for row in KM.kernel_meta(text):
        key = next((k for k in want if k in row['name']), None)
        if key is None:
            continue
        seen.add(key)
        lines, loops = KM.loops(KM.kernel_body(text, row['name']))
        pk = [KM.census('\n'.join(lines[a:b + 1])).get('v_pk', 0) for a, b in loops
              if (lambda c: c.get('lds', 0) <= 4 and c.get('s_load', 0) and c.get('v_pk', 0) > 60)(KM.census('\n'.join(lines[a:b + 1])))]
        pairs, acc = want[key]
        assert pk, key
        # the lifting body's loop is the kernel's leanest source loop (the other body rotates in 4 instructions)
        assert min(pk) <= pairs * (acc + 2), (key, sorted(set(pk)))
        assert min(pk) >= pairs * acc, (key, sorted(set(pk)))
    assert seen == set(want)
