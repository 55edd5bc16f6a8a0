"""
Literal import drop-in (opt-in: `<repo>/compat` on sys.path): `from precise_runner import PreciseRunner`
(the reference's runner/precise_runner/__init__.py:1, runner/example.py:17,33-35) and `from precise.network_runner import
Listener` (the reference's precise/scripts/engine.py:32, listen.py:41-50, simulate.py:35-42) resolve to this framework.
The alias modules are one-liners, not components; what is tested is that unchanged reference-side code runs on them.
"""
import os
import subprocess
import sys
import time

from conftest import REPO

COMPAT = os.path.join(REPO, 'compat')


def _env():
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([COMPAT, REPO] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    env['PYTHONDONTWRITEBYTECODE'] = '1'                      # the child leaves no bytecode caches behind
    return env


def test_reference_runner_tests_pass_unchanged_on_the_aliases(tmp_path):
    """The reference's runner unit tests (runner/test/test_runner.py: `from precise_runner import ReadWriteStream` and the
    two cases restated in test_host.TestReadWriteStream), written out as a test module of their own and collected by pytest
    in a fresh interpreter with only `compat/` in front of the path."""
    import inspect
    from test_host import TestReadWriteStream
    cases = ''.join(inspect.getsource(getattr(TestReadWriteStream, n)) + '\n' for n in ('test_read_write', 'test_chop'))
    module = tmp_path / 'test_runner.py'
    module.write_text('from precise_runner import ReadWriteStream\n\n\nclass TestReadWriteStream:\n' + cases)
    res = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-p', 'no:cacheprovider', '--rootdir', str(tmp_path), str(module)],
                         cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert '2 passed' in res.stdout, res.stdout


def test_reference_side_code_runs_on_the_aliases(tmp_path):
    """A fresh interpreter with `compat/` on its path: the imports of runner/example.py, scripts/engine.py, listen.py and
    simulate.py verbatim; the reference's ReadWriteStream assertions (runner/test/test_runner.py) restated; example.py's
    PreciseEngine + PreciseRunner wiring against a child process that speaks the engine protocol."""
    child = tmp_path / 'fake_engine.py'
    child.write_text(
        "import sys\n"
        "chunk = int(sys.argv[2])\n"
        "n = 0\n"
        "while True:\n"
        "    data = sys.stdin.buffer.read(chunk)\n"
        "    if len(data) < chunk:\n"
        "        break\n"
        "    n += 1\n"
        "    sys.stdout.write(('0.875' if 3 <= n <= 9 else '0.125') + '\\n')\n"
        "    sys.stdout.flush()\n")
    script = tmp_path / 'user_code.py'
    script.write_text(
        "import sys, time\n"
        "from precise_runner import PreciseRunner, PreciseEngine, ReadWriteStream          # runner/example.py:17\n"
        "from precise_runner.runner import ListenerEngine, TriggerDetector                 # listen.py:42, simulate.py:35\n"
        "from precise.network_runner import Listener                                       # scripts/engine.py:32\n"
        "from precise.params import pr, inject_params                                      # simulate.py:39\n"
        "from precise.util import buffer_to_audio                                          # listen.py:50\n"
        "from precise.vectorization import vectorize_raw                                   # simulate.py:42\n"
        "from precise.threshold_decoder import ThresholdDecoder\n"
        "from precise.functions import sigmoid, asigmoid, pdf\n"
        "import precise, precise_runner, precise.params, mycroft_precise_amd.params\n"
        "assert precise.params is mycroft_precise_amd.params                               # ONE `pr` global, as in the reference\n"
        "assert pr.window_samples == 1600 and pr.n_features == 29\n"
        "assert precise_runner.__version__ == '0.3.1'\n"
        "s = ReadWriteStream(b'1234567890')                                                # runner/test/test_runner.py, restated\n"
        "assert s.read(2) == b'12' and s.read(2) == b'34'\n"
        "s.write(b'hi'); assert s.read() == b'567890hi'\n"
        "s.write(b'hello'); assert s.read() == b'hello'\n"
        "assert s.read(1, timeout=0.1) == b''\n"
        "s = ReadWriteStream(chop_samples=10); s.write(b'1234567890hello'); assert s.read(5) == b'hello'\n"
        "preds, acts = [], []\n"
        "engine = PreciseEngine([sys.executable, sys.argv[1]], 'model.pb')                 # runner/example.py:33\n"
        "stream = ReadWriteStream()\n"
        "runner = PreciseRunner(engine, on_prediction=preds.append, on_activation=lambda: acts.append(len(preds)),\n"
        "                       trigger_level=0, stream=stream)                            # runner/example.py:34-35\n"
        "runner.start()\n"
        "stream.write(b'\\0' * 2048 * 12)\n"
        "t0 = time.time()\n"
        "while len(preds) < 12 and time.time() - t0 < 20: time.sleep(0.01)\n"
        "runner.stop()\n"
        "assert preds[:4] == [0.125, 0.125, 0.875, 0.875], preds\n"
        "assert acts and acts[0] == 3, acts                                                # trigger_level 0: first hot chunk fires\n"
        "print('compat ok')\n")
    res = subprocess.run([sys.executable, str(script), str(child)], cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and 'compat ok' in res.stdout, res.stdout + res.stderr


def test_aliases_are_one_liners():
    """The compat tree must stay what it claims to be: aliases, not code."""
    for root, _, files in os.walk(COMPAT):
        for f in files:
            if not f.endswith('.py'):
                continue
            body = [l for l in open(os.path.join(root, f)).read().split('"""')[-1].splitlines() if l.strip() and not l.strip().startswith('#')]
            # (scripts/engine.py: two more lines -- under `python -m` the alias itself is __main__ and must call main())
            assert len(body) <= (6 if f == 'engine.py' else 4), (f, body)
