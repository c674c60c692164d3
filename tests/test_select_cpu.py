"""The parts of the per-guide selection (vsc_search_select) that need no device: the fixed-point floor helper, the
vsc_select struct, the two entry points of the built library, and guide_summary's -K / -S / -T argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(os.environ.get("VSC_TEST_BIN") or os.path.join(ROOT, "varscot_amd", "bin"), "guide_summary")  # (tools/sanitize_cpu.sh)


def test_mit_fixed_is_the_smallest_score_not_below():
    assert va.mit_fixed(0) == 0
    assert va.mit_fixed(1.0) == 2 ** 24
    assert va.mit_fixed(100.0) == int(np.rint(100.0 * 2 ** 24))
    assert va.mit_fixed(0.5) == 2 ** 23
    for x in (0.1, 0.9, 33.3333, 1e-9):
        f = va.mit_fixed(x)
        assert f * 2.0 ** -24 >= x > (f - 1) * 2.0 ** -24


def test_select_struct_layout():
    assert C.sizeof(va.SELECT) == 16
    s = va.SELECT()
    s.top_k, s.min_score = 100, va.mit_fixed(0.1)
    assert bytes(s) == np.array([100, va.mit_fixed(0.1), 0, 0], dtype="<u4").tobytes()


def test_select_symbols_are_bound():
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"vsc_search_select", "vsc_multi_search_select"} <= names
    L = va.lib()
    for n in ("vsc_search_select", "vsc_multi_search_select"):
        fn = getattr(L, n)
        assert fn.restype is C.c_int and len(fn.argtypes) == 9
    header = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    assert "} vsc_select;" in header and "#define VSC_ABI_VERSION 5" in header


def test_select_without_a_context_is_refused():
    h = C.c_void_p()
    sel = va.SELECT()
    p = _lib.SearchParams()
    assert va.lib().vsc_search_select(None, None, None, 0, C.byref(p), C.byref(sel), None, None, C.byref(h)) == -22
    assert va.lib().vsc_multi_search_select(None, None, None, 0, C.byref(p), C.byref(sel), None, None, C.byref(h)) == -22


def test_python_rejects_values_that_do_not_fit():
    from varscot_amd import api
    with pytest.raises(ValueError):
        api._select(-1, 0)
    with pytest.raises(ValueError):
        api._select(0, 2 ** 32)


@pytest.mark.parametrize("extra", [["-K", "x"], ["-K", "-1"], ["-S", "-0.1"], ["-K", "3"], ["-S", "0.5"],
                                   ["-K", "3", "-T", "out.sam"]])
def test_guide_summary_argument_errors(tmp_path, extra):
    """Bad -K / -S values, -K or -S without -T and a -T file of the wrong kind end the tool with status 1 before any
    file or device is opened."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    extra = [str(tmp_path / a) if a.startswith("out.") else a for a in extra]
    r = subprocess.run([TOOL, "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "3", "-R", str(tmp_path / "r.fa")] + extra,
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1
    assert "ERROR" not in r.stderr and r.stderr.startswith(TOOL + ":"), r.stderr  # an argument message, not a failed run


def test_guide_summary_help_lists_the_options():
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("-K, --top", "-S, --min-score", "-T, --hits"):
        assert opt in r.stdout
