"""bench.py's command line and its `--dump-outputs` writer, on CPU: a plain run times ONE region of K steps unless asked otherwise, `--full`
brings the repetitions back, and the dump is float32, capped at 64 MB, and the same sample every time."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_plain_and_full_defaults():
    plain = bench.parse_args(['--steps', '123', '--warmup', '7'])
    assert not plain.full and plain.reps == 1 and plain.steps == 123 and plain.warmup == 7 and plain.dump_outputs is None
    full = bench.parse_args(['--full'])
    assert full.full and full.reps == 5 and full.steps == 5000 and full.warmup == 300
    assert bench.parse_args(['--reps', '3']).reps == 3 and bench.parse_args(['--dump-outputs', 'd']).dump_outputs == 'd'


def test_dump_writes_float32_arrays_as_they_are_below_the_cap(tmp_path):
    rng = np.random.RandomState(0)
    arrays = {'soc': rng.rand(17, 64).astype(np.float32), 'district': rng.rand(4, 64)}
    shapes = bench.write_outputs(arrays, tmp_path / 'out')
    assert shapes == {'soc': [17, 64], 'district': [4, 64]}
    for name, a in arrays.items():
        got = np.load(tmp_path / 'out' / f'{name}.npy')
        assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))


def test_dump_above_the_cap_is_a_fixed_sample_within_it(tmp_path):
    rng = np.random.RandomState(1)
    arrays = {'net': rng.rand(17, 4096).astype(np.float32), 'reward': rng.rand(17, 4096).astype(np.float32)}
    cap = 100_000
    bench.write_outputs(arrays, tmp_path / 'a', budget=cap)
    bench.write_outputs(arrays, tmp_path / 'b', budget=cap)
    assert sum(f.stat().st_size for f in (tmp_path / 'a').iterdir()) <= cap
    for name, a in arrays.items():
        x, y = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert x.dtype == np.float32 and x.ndim == 1 and 0 < x.size < a.size and np.array_equal(x, y)
        assert np.isin(x, a.reshape(-1)).all()                 # elements of the array, not anything derived from them
