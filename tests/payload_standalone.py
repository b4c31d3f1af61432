"""tests/payload_validate_main.cc built with the host compiler and -fsanitize=address,undefined, and
one run of it over a corpus — TEST INFRASTRUCTURE shared by test_wire_host.py, test_sign_host.py
and test_qsgd_ef_host.py (``from payload_standalone import standalone, run``).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_built = None


def _compiler():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return c
    raise RuntimeError("no host C++ compiler")


@pytest.fixture(scope="module")
def standalone(tmp_path_factory):
    """(path of the program, sanitized?): built once per session with
    -fsanitize=address,undefined, or without when the sanitizer runtime does not link on this
    machine."""
    global _built
    if _built is None:
        d = tmp_path_factory.mktemp("payload_validate")
        exe = str(d / "payload_validate_main")
        src = os.path.join(ROOT, "tests", "payload_validate_main.cc")
        base = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", src, "-o", exe]
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
        # the runtimes linked into the program itself where the compiler can (the program then
        # starts whatever else the loader brings in first)
        for extra in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
            r = subprocess.run(base + san + extra, capture_output=True, text=True)
            if r.returncode == 0:
                _built = exe, True
                break
        else:
            print("sanitizer build failed, building without:\n" + r.stderr[-2000:])
            subprocess.run(base, check=True)
            _built = exe, False
    return _built


def run(exe, args, tmp_path, corpus):
    """The program's output lines, one per entry ``(name, bytes, n_expected, ...)`` of ``corpus``;
    ``args``: the kind, then ``--trunc`` or ``--clamp`` if wanted.  Fails on a sanitizer report."""
    lines = []
    for i, (_, raw, n_expected, *_) in enumerate(corpus):
        path = tmp_path / f"payload_{i:03d}.bin"
        path.write_bytes(raw)
        lines.append(f"{n_expected} {path}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args, str(tmp_path / "list.txt")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert len(out) == len(corpus)
    return out
