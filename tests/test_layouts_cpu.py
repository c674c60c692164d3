"""vsc_timing.seed_layout without a GPU: the field took the place of the struct's reserved word (same size, same ABI
version), the Python mirror reads it there, and tests/layouts.py decodes the bits the header documents."""
import ctypes as C
import os
import re

from varscot_amd import _lib
from layouts import LAYOUTS, decode, named

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seed_layout_is_the_last_word_of_vsc_timing():
    header = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} vsc_timing;", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    assert fields == [name for name, _ in _lib.Timing._fields_] and fields[-1] == "seed_layout"
    assert C.sizeof(_lib.Timing) == 136 and _lib.Timing.seed_layout.offset == 132 == _lib.Timing.seed_cut.offset + 4
    assert "seed_layout" in _lib.Timing().as_dict()


def test_decode_reads_the_documented_bits():
    assert decode(0) == dict(shared=False, group_out=False, fill=False, reserve_log2=0, launches=0)  # a scan
    assert decode(1 | 2 | (10 << 4) | (1 << 8)) == dict(shared=True, group_out=True, fill=False, reserve_log2=10, launches=1)
    assert decode(1 | 4 | (6 << 4) | (64 << 8)) == dict(shared=True, group_out=False, fill=True, reserve_log2=6, launches=64)
    assert named("wave") == dict(shared=False, group_out=False)
    assert named("wave-1024") == dict(shared=False, group_out=False, reserve_log2=10)
    assert named("group-64") == dict(shared=True, group_out=True, reserve_log2=6)
    assert named("shared-wave-out") == dict(shared=True, group_out=False)
    assert sorted(LAYOUTS) == ["group", "group-1024", "group-64", "shared-wave-out", "wave", "wave-1024", "wave-64"]
