"""`bin/optimizer`'s transcripts, pinned: per command the exit status, the sha256 of stdout (the program) and the log stream with
only times, rates and thread counts replaced by a token -- every other byte, the ANSI colour codes included, is compared as it
is.  No device is needed: the rows use `--gpu 0`, or run a copy of the tool that finds no library and pin what it says then.

The fixture `golden/optimizer_transcripts.json` is recorded from the tool as built from the commit BEFORE a change of the tool's
structure, by `python tests/test_optimizer_transcripts_host.py --record [path of that optimizer]`; the recording runs every
command twice and refuses to write a fixture whose two runs differ.  Its "recorded_from" names the commit."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
OPT = os.path.join(ROOT, "bin", "optimizer")
FIXTURE = os.path.join(ROOT, "tests", "golden", "optimizer_transcripts.json")

FLOAT = r"[0-9]+(?:\.[0-9]+)?(?:e[+-]?[0-9]+)?"
# what differs from run to run: times, rates, thread counts.  Nothing else is replaced.
PATTERNS = [
    (re.compile(r"in %s s on [0-9]+ threads" % FLOAT), "in <T> s on <N> threads"),          # host search
    (re.compile(r"\t%ss$" % FLOAT, re.M), "\t<T>s"),                                        # the additions line
    (re.compile(r"kernel %s ms" % FLOAT), "kernel <T> ms"),
    (re.compile(r"in %s ms" % FLOAT), "in <T> ms"),
    (re.compile(r"%s candidates/s" % FLOAT), "<R> candidates/s"),
    (re.compile(r"index %s s, candidate %s s" % (FLOAT, FLOAT)), "index <T> s, candidate <T> s"),   # --engine fast
]

Q = ["-q", "131071"]
WL, WR, WP, L3 = ("2x2x2_7_Winograd_L.sms", "2x2x2_7_Winograd_R.sms", "2x2x2_7_Winograd_P.sms", "3x3x3_23_58_L.sms")
FULLRANK = "3 3 M\n1 1 1\n1 2 1\n2 2 1\n2 3 -1\n3 1 1\n3 3 2\n0 0 0\n"      # rows 1 1 0 / 0 1 -1 / 1 0 2: no kernel
H = ["--gpu", "0"]

# (id, arguments before the matrix, matrix, extra environment)
CASES = [
    ("default_DKG", Q + H + ["-O", "200"], WL, {}),
    ("A_E_N", Q + H + ["-O", "64", "-A", "-E", "-N"], WL, {}),
    ("rationals", H + ["-O", "50"], WR, {}),
    ("modulus_above_2_31", ["-q", "4611686018427387847"] + H + ["-O", "20", "--only", "K"], WL, {}),
    ("K_F", Q + H + ["-O", "40", "-K", "-F"], WP, {}),
    ("K_blocks_of_4", Q + H + ["--only", "K", "--kernel-block", "4", "-O", "10"], L3, {}),
    ("E_15120_schedules", Q + H + ["--only", "E", "-O", "10"], L3, {}),
    ("E_recsub", Q + H + ["--only", "E", "--recsub", "-O", "10"], WR, {}),
    ("N_orders_5_7", Q + H + ["--only", "N", "--orders", "5:7", "-O", "10"], WL, {}),
    ("orders_past_the_end", Q + H + ["--only", "N", "--orders", "5040:1"], WL, {}),
    ("orders_without_N", Q + H + ["--only", "D", "--orders", "1:1"], WL, {}),
    ("orders_malformed", Q + H + ["--orders", "3"], WL, {}),
    ("zero_dimensional_kernel", Q + H + ["-O", "10"], None, {}),
    ("A_fewer_rows_than_columns", Q + H + ["--only", "A"], WP, {}),
    ("N_23_rows", Q + H + ["--only", "N"], L3, {}),
    ("replay_only", Q + H + ["--seed", "3", "--replay"], WL, {}),
    ("engine_literal", Q + H + ["-O", "200", "--engine", "literal"], WL, {}),
    ("engine_fast", Q + H + ["-O", "200", "--engine", "fast"], WL, {}),
    ("forked_shards_host_engine", Q + ["--gpu", "2", "--only", "D", "-O", "40"], WL, {"PLO_SHARD_ENGINE": "host"}),
]
# run by a copy of the tool with no library beside it and none named in the environment
NOLIB = [
    ("nolib_D", Q + ["--gpu", "1", "-O", "10", "--only", "D"], WL),
    ("nolib_G", Q + ["--gpu", "1", "-O", "10", "--only", "G"], WL),
    ("nolib_A", Q + ["--gpu", "1", "-O", "10", "--only", "A"], WL),
    ("nolib_K", Q + ["--gpu", "1", "-O", "10", "--only", "K"], WL),
    ("nolib_N", Q + ["--gpu", "1", "-O", "10", "--only", "N"], WL),
    ("nolib_N_orders", Q + ["--gpu", "1", "-O", "10", "--only", "N", "--orders", "0:5"], WL),
    ("nolib_E", Q + ["--gpu", "1", "-O", "10", "--only", "E"], WL),
    ("nolib_2_shards_D", Q + ["--gpu", "2", "-O", "10", "--only", "D"], WL),
    ("nolib_2_shards_K", Q + ["--gpu", "2", "-O", "10", "--only", "K"], WL),
]


def normalise(err):
    for pat, token in PATTERNS:
        err = pat.sub(token, err)
    return err


def transcript(tool, args, matrix, extra_env, workdir, drop=()):
    if matrix is None:
        path = os.path.join(workdir, "fullrank.sms")
        with open(path, "w") as fh:
            fh.write(FULLRANK)
    else:
        path = os.path.join(DATA, matrix)
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(extra_env)
    r = subprocess.run([tool] + args + [path], capture_output=True, env=env, timeout=120)
    return {"status": r.returncode, "stdout_sha256": hashlib.sha256(r.stdout).hexdigest(), "stderr": normalise(r.stderr.decode())}


def lone_copy(tool, workdir):
    """a copy of the tool in a directory of its own: neither place beside the executable holds the library"""
    d = os.path.join(workdir, "lone", "bin")
    os.makedirs(d, exist_ok=True)
    return shutil.copy(tool, os.path.join(d, "optimizer"))


NOLIB_DROP = ("PLO_HIP_LIB", "PLINOPT_HIP_LIB", "LD_LIBRARY_PATH")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "plinopt_amd", "csrc", "host")])


@pytest.fixture(scope="module")
def pinned():
    with open(FIXTURE) as fh:
        return json.load(fh)["transcripts"]


def test_every_case_is_pinned(pinned):
    assert sorted(pinned) == sorted([c[0] for c in CASES] + [c[0] for c in NOLIB])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_transcript(case, pinned, tmp_path):
    name, args, matrix, extra_env = case
    assert transcript(OPT, args, matrix, extra_env, str(tmp_path)) == pinned[name]


@pytest.mark.parametrize("case", NOLIB, ids=[c[0] for c in NOLIB])
def test_transcript_without_a_library(case, pinned, tmp_path):
    name, args, matrix = case
    got = transcript(lone_copy(OPT, str(tmp_path)), args, matrix, {}, str(tmp_path), drop=NOLIB_DROP)
    if "cannot load libplinopt_hip.so" not in got["stderr"]:
        pytest.skip("the loader of this machine finds a libplinopt_hip.so on its own search path")
    assert got == pinned[name]


def record(tool):
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lone = lone_copy(tool, tmp)
        rows = [(n, tool, a, m, e, ()) for n, a, m, e in CASES] + [(n, lone, a, m, {}, NOLIB_DROP) for n, a, m in NOLIB]
        for name, exe, args, matrix, extra_env, drop in rows:
            one, two = (transcript(exe, args, matrix, extra_env, tmp, drop) for _ in range(2))
            if one != two:
                sys.exit("refusing to record: two runs of %s differ\n%r\n%r" % (name, one, two))
            if exe == lone and "cannot load libplinopt_hip.so" not in one["stderr"]:
                sys.exit("refusing to record %s: this machine's loader finds a library" % name)
            out[name] = one
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    with open(FIXTURE, "w") as fh:
        json.dump({"recorded_from": commit, "transcripts": out}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded %d transcripts from %s (commit %s)" % (len(out), tool, commit))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        record(sys.argv[2] if len(sys.argv) > 2 else OPT)
    else:
        sys.exit("usage: %s --record [optimizer built from the commit to pin]" % sys.argv[0])
