"""The layouts the seed search can leave its records in, as hook dicts (include/varscot_hip_debug.h), and what
vsc_timing.seed_layout says about the search that ran (include/varscot_hip.h).  A plain helper module: a test sets a layout's
hooks, runs a call and proves with `check` that the layout it named is the one the call used."""

LAYOUTS = {
    "wave": dict(seed_shared=0),                                        # a chunk and open blocks per wave
    "wave-64": dict(seed_shared=0, seed_reserve=64),
    "wave-1024": dict(seed_shared=0, seed_reserve=1024),
    "group": dict(seed_shared=1, seed_group_out=1),                     # a chunk and open blocks per workgroup (the c3 shape)
    "group-64": dict(seed_shared=1, seed_group_out=1, seed_reserve=64),
    "group-1024": dict(seed_shared=1, seed_group_out=1, seed_reserve=1024),
    "shared-wave-out": dict(seed_shared=1, seed_group_out=0),           # a chunk per workgroup, open blocks per wave
}


def decode(seed_layout):
    """vsc_timing.seed_layout in words."""
    v = int(seed_layout)
    return dict(shared=bool(v & 1), group_out=bool(v & 2), fill=bool(v & 4), reserve_log2=(v >> 4) & 15, launches=(v >> 8) & 255)


def named(name):
    """What decode() must show of the layout `name` (reserve_log2 only where the layout sets the block size)."""
    hooks = LAYOUTS[name]
    shared = hooks["seed_shared"] == 1
    want = dict(shared=shared, group_out=shared and hooks.get("seed_group_out", -1) != 0)
    if "seed_reserve" in hooks:
        want["reserve_log2"] = hooks["seed_reserve"].bit_length() - 1
    return want


def check(timing, name, fill, launches=1):
    """The call behind `timing` (ctx.timing()) ran a seed search in the layout `name`, with the block fill table or with
    sentinels, in `launches` launches.  Returns the decoded layout."""
    assert timing["algorithm"] == 2, timing  # VSC_ALGO_SEED: a scan has no layout
    got = decode(timing["seed_layout"])
    want = dict(named(name), fill=bool(fill), launches=launches)
    assert {k: got[k] for k in want} == want, (name, got)
    assert 6 <= got["reserve_log2"] <= 10, got
    return got
