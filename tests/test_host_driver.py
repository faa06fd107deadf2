"""The host half of the propagate drivers that needs no device: where the regions
of a propagate's one device allocation lie (csrc/prop_layout.h, used by prop_bufs
and launch_step) and the grow step of the per-thread device buffers
(csrc/grow_buffer.h, used by every pool_get).

tests/host_driver_check.cpp is compiled for the host against those two headers --
the text propagate.hip compiles -- and run.  Layouts: photon counts 1, 63, 64, 65,
4095, 4096, 4097, 2^20 - 1, 2^20, 2^20 + 1 and 10^7; 64 x 64, 100 x 41 (not fused)
and 512 x 1024 slots; sort temporaries of 0, 1 and 2^26 bytes; with and without
tail masks; a step over all, half or one of the photons, placed as a
device-driven slot and as a host step places it.  Every region inside the total,
aligned as its user casts it (16: scratch, hits; 256: sort space, temporary,
rays, live records, tail masks; 8: the mask words), as large as its user touches,
and disjoint from every other.  Buffer: a failed grow after a successful one
returns the error, the next smaller request does not succeed with a null
pointer, and a request that fits allocates nothing.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chroma-lite_amd', 'csrc')


def _compiler():
    for c in ('c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++'):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('host_driver') / 'host_driver_check')
    subprocess.check_call([_compiler(), '-O2', '-std=c++17', '-Wall', '-I', CSRC, '-o', exe,
                           os.path.join(ROOT, 'tests', 'host_driver_check.cpp')])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    line = p.stdout.strip().splitlines()[-1]
    print(line)
    d = dict(kv.split('=', 1) for kv in line.split())
    d['returncode'] = p.returncode
    return d


def test_layout_and_pool(report):
    assert int(report['layouts']) == 11 * 4 * 3 * 2 * 3 * 2
    assert int(report['violations']) == 0, 'first violation: %s' % report['first_violation']
    assert report['returncode'] == 0
