"""The padded one-FMA slab planes of the wide-node test never cull what the
two-FMA planes enter (csrc/slab_plane.h has the proof; this is the check).

tests/slab_pad_check.cpp is compiled for the host against that header -- the text
the kernels compile -- and run: >= 10^7 random planes plus an adversarial grid
(bytes 0..255; node origins, exponents as quantize_axis picks them, for worlds of
1 mm .. 10^6 mm; ray origins inside, on the faces and up to 10x outside; direction
components 0, denormal, smallest normal, 1e-33 .. 1e-3, (0.1, 1], both signs;
origins a few ulps from the plane, where org * inv cancels noid).  Float FMA is the
host's fmaf, not an emulation.

Asserted, with no exclusions: for every plane T'_near(padded) <= T(two-step) <=
T'_far(padded); every value finite unless the axis is wild (pad +inf), where the
padded distances are -inf/+inf or NaN, which the fmaxf/fminf chains ignore (that
rule is checked too); no drawn node lies outside the bound wide_validate enforces.
The largest |T - T'(unpadded)| / eps must stay <= 0.5: the proof bounds the
unpadded difference by 4u M and the pad is 8u M (the padded claim itself needs
5u M, so 1.6x slack).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chroma-lite_amd', 'csrc')
RATIO_LIMIT = 0.5


def _compiler():
    for c in ('c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++'):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('slab_pad') / 'slab_pad_check')
    subprocess.check_call([_compiler(), '-O2', '-std=c++17', '-ffp-contract=off', '-I', CSRC, '-o', exe,
                           os.path.join(ROOT, 'tests', 'slab_pad_check.cpp'), '-lm'])
    p = subprocess.run([exe, '10000000', '20240611'], stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
    line = p.stdout.strip().splitlines()[-1]
    print(line)
    d = dict(kv.split('=', 1) for kv in line.split())
    d['returncode'] = p.returncode
    return d


def test_padded_planes_enclose_two_step(report):
    assert int(report['random_planes']) >= 10 ** 7 and int(report['grid_planes']) > 10 ** 6
    assert int(report['violations']) == 0, 'first counter-example (q, s, org, o, d, W): %s' % report['first_violation']
    assert int(report['nonfinite']) == 0
    assert int(report['outside_bound']) == 0
    assert report['returncode'] == 0


def test_wild_axes_drawn_and_nan_rule(report):
    # the extreme reciprocals are in the draw (and pass above as never-culling), and
    # fmax/fmin skip a NaN operand, all-NaN included
    assert int(report['wild']) > 10 ** 5
    assert int(report['nan_rule']) == 1


def test_unpadded_difference_within_half_pad(report):
    print('max |T - T\'| / eps = %s, largest pad in space %s mm' % (report['max_ratio'], report['max_pad_mm']))
    assert 0.0 < float(report['max_ratio']) <= RATIO_LIMIT
