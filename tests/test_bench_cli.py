"""bench.py's process set-up, without a GPU: MIOpen's user databases are a private copy of
miopen_cache/ (MIOpen opens them read-write, and a checkout may be read-only), removed at exit."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = ("import os, bench; d = os.environ['MIOPEN_USER_DB_PATH']; "
        "print(d); print(os.environ['MIOPEN_CUSTOM_CACHE_DIR']); print(','.join(sorted(os.listdir(d))))")


def _import_bench(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIOPEN_")}
    env.update(extra)
    r = subprocess.run([sys.executable, "-c", CODE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()[-3:]


def _committed_cache():
    d = os.path.join(ROOT, "miopen_cache")
    return {f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d)}


def test_miopen_databases_are_a_private_copy():
    before = _committed_cache()
    db, cache, files = _import_bench()
    assert db == cache and os.path.commonpath([ROOT, os.path.realpath(db)]) != ROOT
    assert files.split(",") == sorted(before)
    assert not os.path.exists(db)  # removed when the process ended
    assert _committed_cache() == before


def test_miopen_paths_of_the_caller_are_kept(tmp_path):
    db, cache, files = _import_bench(MIOPEN_USER_DB_PATH=str(tmp_path), MIOPEN_CUSTOM_CACHE_DIR=str(tmp_path))
    assert db == cache == str(tmp_path) and files == ""
