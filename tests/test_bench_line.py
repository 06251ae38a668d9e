"""CPU checks of what bench.py SAYS about itself (the headline line named fp32-input MFMA while the shipped
variant 9 multiplies on split-f16)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('lemo_bench', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize('variant', list(range(0, 12)))
def test_arithmetic_label_names_the_scheme_that_runs(variant):
    label = _bench().arithmetic_label(variant)
    if variant >= 4:
        assert 'split-f16' in label and 'fp16 pieces' in label and 'fp32-input MFMA' not in label
    elif variant == 3:
        assert 'bf16 pieces' in label
    else:
        assert 'fp32-input MFMA' in label


def test_default_variant_label_is_split_f16():
    b = _bench()
    from lemo_amd.priors import DEFAULT_CONV_VARIANT
    assert b.DEFAULT_CONV_VARIANT == DEFAULT_CONV_VARIANT
    assert 'split-f16' in b.arithmetic_label(DEFAULT_CONV_VARIANT)


def _bench_dump(out_dir, steps, warmup, extra=()):
    """``bench.py --gpus 1 --emu --steps K --warmup W --dump-outputs DIR`` (the host-emulated library): the JSON line and the arrays"""
    import json
    import subprocess
    import sys
    import numpy as np
    subprocess.run(['make', '-C', os.path.join(ROOT, 'lemo_amd', 'csrc'), '-j8', 'emu'], check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--emu', '--backend', 'gloo', '--steps', str(steps),
           '--warmup', str(warmup), '--dump-outputs', str(out_dir)] + list(extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(env, OMP_NUM_THREADS='2'))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.timeout(900)
def test_dump_outputs_hold_the_last_timed_step(tmp_path, emu_lib):
    """--dump-outputs writes what the timed path computed in its last step (float32 / float64, at most 64 MB), the same arguments give
    the same arrays, and --steps K after --warmup W is exactly W + K iterations of the fit"""
    import numpy as np
    d, a = _bench_dump(tmp_path / 'a', 3, 1)
    assert d['steps'] == 3 and d['warmup'] == 1 and d['ms_per_step'] > 0
    assert {'params72', 'params75', 'vertices', 'joints', 'loss_total'} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert float(a['loss_total']) == np.float32(d['final_total_loss'])
    _, b = _bench_dump(tmp_path / 'b', 3, 1)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # the same fit in this process: W warm-up + K timed iterations from the seeded start
    fit, _, B = _bench().build_problem_emu(0)
    fit.step(1, use_graph=False)
    fit.step(3, use_graph=False)
    assert a['params72'].shape == (1, B, 72)
    assert np.array_equal(a['params72'][0], fit.params72().numpy())
    assert np.array_equal(a['params75'], fit.params75().numpy())
    assert np.array_equal(a['vertices'], fit.vertices().numpy())
    fit.step(1, use_graph=False)
    assert not np.array_equal(a['params72'][0], fit.params72().numpy())      # one more step is visible


@pytest.mark.timeout(900)
def test_dump_outputs_prox_workload(tmp_path, emu_lib):
    import numpy as np
    d, a = _bench_dump(tmp_path / 'p', 2, 1, ['--workload', 'prox'])
    assert d['steps'] == 2 and d['ms_per_step'] > 0
    assert a['params'].shape[0] == 1 and a['params'].dtype == np.float32 and np.isfinite(a['params']).all()
    assert float(a['total_loss']) == np.float32(d['total_loss'])


# what only ``--full`` measures: a plain run carries none of it
FULL_ONLY_KEYS = ('value_100_steps', 'stage_us', 'roofline', 'concurrent_clips', 'variants', 'mpjpe', 'mpjpe_mm', 'coherent_model',
                  'prox_window', 'perframe', 'ae_finetune', 'cpu_baseline', 'speedup_vs_cpu_baseline')


def test_full_is_off_by_default():
    ap = _bench().arg_parser()
    assert ap.parse_args([]).full is False
    assert ap.parse_args(['--full']).full is True


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_run_is_the_headline_alone():
    """``bench.py --gpus 1 --steps K --warmup W`` prints the headline line and does nothing beyond it"""
    import json
    import subprocess
    import sys
    import time
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)],
                         capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['metric'] == 'fitting-iterations/sec (T=120 frames)' and d['unit'] == 'fitting-iterations/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32' and d['steps'] == steps and d['warmup'] == warmup and d['value'] > 0
    assert abs(d['ms_per_step'] - 1e3 / d['value']) <= 1e-6 * d['ms_per_step']
    assert not set(FULL_ONLY_KEYS) & set(d), sorted(set(FULL_ONLY_KEYS) & set(d))
    print(f'\nplain bench run: {wall:.1f} s wall, {wall - (steps + warmup) * d["ms_per_step"] * 1e-3:.1f} s outside the steps')
