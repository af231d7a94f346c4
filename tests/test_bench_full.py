"""bench.py --full: a plain run reports the headline alone, --full adds the measurements beside it; the headline's fields are the same in both."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ARGS = ['--stub-model', '--steps', '2', '--warmup', '1', '--batch', '3', '--total', '4']
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'n_gpus', 'scaling')


def _line(capsys, extra):
    out = bench.run(ARGS + extra)
    printed = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(printed) == 1 and json.loads(printed[0]) == out
    return out


def test_a_plain_run_reports_the_headline_alone(capsys):
    plain = _line(capsys, [])
    assert plain['full'] is False and plain['configs2_strong_64'] is None
    assert plain['steps'] == 2 and plain['warmup'] == 1 and plain['value'] > 0
    # 3 sequences per step at 2 ms each: value and ms_per_step describe the same timed steps
    assert abs(plain['ms_per_step'] * plain['value'] / 1e3 - 3) < 1e-6


def test_full_adds_the_other_lines_and_leaves_the_headline_fields(capsys):
    plain, full = _line(capsys, []), _line(capsys, ['--full'])
    assert full['full'] is True
    strong = full['configs2_strong_64']
    assert strong['scaling'] == 'strong' and strong['sequences_total'] == 4 and strong['sequences_per_sec'] > 0
    for k in HEADLINE:
        assert k in plain and k in full
        if k not in ('value', 'ms_per_step'):
            assert plain[k] == full[k], k
    # each of the lines that moved keeps its own switch under --full
    assert _line(capsys, ['--full', '--no-strong-line'])['configs2_strong_64'] is None
