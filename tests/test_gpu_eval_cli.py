"""The icp-gpu CLI's --evaluate, --evaluate-both and --write-information on the cow pair: the lines carry
the Python call's numbers at the pose the run reached, the matrix round-trips through its CSV, and the
flags only ADD lines: a run of this program with them prints, but for the [evaluate] lines, and writes to
its output file exactly what a run of this program without them does.  (That the flag-less output is the
program's of before the flags existed is not something a test of one binary can show: it rests on the
flag-less path of icp_cli.cpp, which takes none of the new branches.)"""
import math
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the session: torch then sees the device)

import datasets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iterative-closest-point_amd", "build", "icp-gpu")
DIST = 0.1


def g(v):
    return float("%g" % v)


def run(args, cwd):
    return subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def test_evaluate_lines_and_the_information_file(icp_lib, tmp_path):
    amd = icp_lib
    ref, tr = datasets.path("cow_ref"), datasets.path("cow_tr1")
    info, out, out0 = str(tmp_path / "info.txt"), str(tmp_path / "out.txt"), str(tmp_path / "out0.txt")
    plain = run([ref, tr, "5", "--out", out0], tmp_path)
    r = run([ref, tr, "5", "--evaluate", str(DIST), "--evaluate-both", "--write-information", info, "--out", out], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("[evaluate]")]
    print("\n".join(lines))
    assert len(lines) == 2 and lines[0].startswith("[evaluate] scene ") and lines[1].startswith("[evaluate] model ")
    # without the flags: no such line, and everything else is the same
    assert "[evaluate]" not in plain.stderr and plain.stdout == r.stdout
    rest = [l for l in r.stderr.splitlines() if not l.startswith("[evaluate]")]
    assert rest == [l.replace(out0, out) for l in plain.stderr.splitlines()]
    with open(out, "rb") as a, open(out0, "rb") as b:
        assert a.read() == b.read()
    # the numbers are the Python call's at the same pose
    m, p = amd.load_matrix(ref), amd.load_matrix(tr)
    with amd.Context() as c:
        c.set_model(m)
        c.set_scene(p)
        c.run(5)
        ev = c.evaluate(DIST, both=True)
    for line, pre in zip(lines, ("", "model_")):
        w = line.split()
        K = ev[pre + "correspondences"] if pre else ev["correspondences"]
        n = ev[pre + "points"] if pre else ev["scene_points"]
        rmse = ev["model_rmse"] if pre else ev["inlier_rmse"]
        assert (int(w[2]), int(w[4]), float(w[6].rstrip(","))) == (K, n, g(DIST))
        assert float(w[8]) == g(ev[pre + "fitness"]) and float(w[11]) == g(rmse)
        assert float(w[15]) == g(math.sqrt(ev[pre + "max_inlier_d2"]))
    assert 0 < ev["correspondences"] <= p.shape[0]
    A = np.loadtxt(info, delimiter=",")
    assert A.shape == (6, 6)
    np.testing.assert_array_equal(A, np.vectorize(g)(ev["information"]))
    # a matrix that cannot be written is an error, not a silent exit 0
    r = run([ref, tr, "2", "--evaluate", str(DIST), "--write-information", str(tmp_path / "no_such_dir" / "i.txt"),
             "--out", out], tmp_path)
    assert r.returncode == 2 and "cannot write" in r.stderr
    # forward alone: one line; inf is a distance
    r = run([ref, tr, "2", "--evaluate", "inf", "--out", out], tmp_path)
    lines = [l for l in r.stderr.splitlines() if l.startswith("[evaluate]")]
    assert r.returncode == 0 and len(lines) == 1 and lines[0].split()[2] == lines[0].split()[4] == str(p.shape[0])


def test_the_options_are_checked_before_anything_runs(tmp_path):
    ref, tr = datasets.path("cow_ref"), datasets.path("cow_tr1")
    for args, word in ((["--evaluate", "0"], "--evaluate: 0 is not a distance"), (["--evaluate", "x"], "--evaluate: x"),
                       (["--evaluate-both"], "need --evaluate"), (["--write-information", "i.txt"], "need --evaluate")):
        r = run([ref, tr, "2"] + args, tmp_path)
        assert r.returncode != 0 and word in r.stderr and "[load]" not in r.stderr, (args, r.stderr)
    assert not os.path.exists(tmp_path / "output.txt")
