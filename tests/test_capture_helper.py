"""Contract of the engines' stream-capture helper (lemo_amd/csrc/engine_host.hpp: capture_graph, replay_or_run, destroy_graphs) on its error
paths -- begin / body / end / instantiate / launch failing, upload on and off, capture once then replay -- which no GPU test can reach without provoking a fault.
tests/capture_helper_main.cpp drives the header against the scripted runtime of tests/capture_mock as a stand-alone host program
under the address and undefined-behaviour sanitizers (a graph destroyed twice or leaked ends the run with an error)."""
import os
import shutil
import subprocess

from conftest import CSRC, ROOT

ROCM_CLANG = '/opt/rocm/lib/llvm/bin/clang++'          # the Makefile's HOSTCXX


def test_capture_graph_contract(tmp_path):
    cxx = os.environ.get('HOSTCXX') or (ROCM_CLANG if os.path.exists(ROCM_CLANG) else shutil.which('c++'))
    exe = str(tmp_path / 'capture_helper')
    subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall', '-Wextra',
                    '-Werror', '-I' + os.path.join(ROOT, 'tests', 'capture_mock'), '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC,
                    os.path.join(ROOT, 'tests', 'capture_helper_main.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all capture_graph checks hold' in r.stdout
