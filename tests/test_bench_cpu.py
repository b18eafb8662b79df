"""bench.py's command line and its --dump-outputs writer, without a GPU: the options a plain run and a --full run
take, and the files written for a step's results (float64, one set per query, clock readings left out)."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _result(n_way, n_rows, k):
    r = {name: float(10 * k + i) for i, name in enumerate(bench.DUMP_STATS)}
    r["status"], r["iterations"], r["configs_checked"] = 0, 100 + k, 12345 + k
    r["cost_best"] = [1.5 + k, 2.5, 3.5]
    r["cost_theoretical"] = [0.5, 0.25, 0.125]
    r["path"] = np.arange(n_way * 8, dtype=np.float64).reshape(n_way, 8) + k
    r["cost_rows"] = np.arange(n_rows * 5, dtype=np.float64).reshape(n_rows, 5)
    r["time_total"] = 0.123  # a clock reading: not dumped
    return r


def test_dump_outputs_writes_each_query(tmp_path):
    out = tmp_path / "dump" / "nested"
    results = [_result(4, 3, 0), _result(0, 0, 1)]
    bench.dump_outputs(str(out), [2, 5], results)
    assert sorted(os.listdir(out)) == sorted("q%d_%s.npy" % (q, n) for q in (2, 5)
                                             for n in ("path", "cost_rows", "stats"))
    for qid, r in zip((2, 5), results):
        path = np.load(out / ("q%d_path.npy" % qid))
        rows = np.load(out / ("q%d_cost_rows.npy" % qid))
        stats = np.load(out / ("q%d_stats.npy" % qid))
        assert path.dtype == rows.dtype == stats.dtype == np.float64
        assert np.array_equal(path, r["path"]) and path.shape[1] == 8
        assert np.array_equal(rows, r["cost_rows"][:, [0, 2, 3, 4]]) and rows.shape[1] == 4
        assert len(stats) == len(bench.DUMP_STATS) + 4  # two three-component costs
        i = bench.DUMP_STATS.index("configs_checked")
        assert stats[i] == r["configs_checked"]
        j = bench.DUMP_STATS.index("cost_best")
        assert stats[j:j + 3].tolist() == r["cost_best"] and stats[j + 3:j + 6].tolist() == r["cost_theoretical"]


def test_command_line_defaults(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs, a.no_cpu) == (7, 3, False, None, False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
