"""Which way an ICP registration runs, decided in one place (no GPU: pedp_debug_icp_path calls the library's decision function).

The table below restates the rules from the switches' own descriptions (include/pedp.h):
  fused           units of one tile, no exhaustive sweep, r > 0, both clouds non-empty, at most BK_WCAP mask words of 1024 rows
  copy_bracket    PEDP_ICP_COPY_BRACKET=1 (either path); exchange: a hook or the communicator (either path)
  -- everything below needs the fused path --
  serial_close    PEDP_ICP_SERIAL_CLOSE=1;  unfused_finish: PEDP_ICP_UNFUSED_FINISH=1
  plan            a single registration, unless PEDP_ICP_NO_VISIT_PLAN=1
  certify         a single registration whose passes close themselves (no exchange, no unfused finish), unless PEDP_ICP_CERT=0
  dev_result      a single registration, not a batch group, whose passes close themselves, unless PEDP_ICP_COPY_BRACKET=1
  head            dev_result, the wide close, unless PEDP_ICP_HEAD_CLOSE=0
  steady          head and certify, unless PEDP_ICP_STEADY=0; timed_pass -1 or -3; no early-exit look; the caller allows it; resident
"""
import itertools

import pytest

BK_WCAP = 512            # csrc/icp/fused_close.h: mask words the fused pass lists in LDS
ELIGIBLE = dict(n_source=1000, n_target=5000, radius=1.0, unit_size=1, poses=1, timed_pass=-1, resident=True)


def expected(on, steady_from=5, n_source=1, n_target=1, radius=1.0, unit_size=1, poses=1, timed_pass=-1, exhaustive=False,
             exchange=False, early_exit=False, no_steady=False, resident=False, batch=False):
    on = set(on)
    e = dict.fromkeys(("fused", "dev_result", "copy_bracket", "head", "certify", "plan", "serial_close", "unfused_finish",
                       "exchange", "steady"), False)
    e["steady_from"] = max(1, steady_from)
    e["copy_bracket"] = "copy_bracket" in on
    e["exchange"] = exchange
    e["fused"] = (unit_size == 1 and not exhaustive and radius > 0 and n_source > 0 and n_target > 0
                  and (n_target + 1023) // 1024 <= BK_WCAP)
    if not e["fused"]:
        return e
    single = poses <= 1
    closes_itself = not exchange and "unfused_finish" not in on
    e["serial_close"] = "serial_close" in on
    e["unfused_finish"] = "unfused_finish" in on
    e["plan"] = single and "no_visit_plan" not in on
    e["certify"] = single and closes_itself and "cert" in on
    e["dev_result"] = single and not batch and closes_itself and "copy_bracket" not in on
    e["head"] = e["dev_result"] and "serial_close" not in on and "head_close" in on
    e["steady"] = (e["head"] and e["certify"] and "steady" in on and timed_pass in (-1, -3) and not early_exit and not no_steady
                   and resident)
    return e


def check(on, **kw):
    from pedp_hip import _lib

    got = _lib.icp_path(on, **kw)
    assert got == expected(on, **kw), (sorted(on), kw)
    return got


DEFAULT = ("head_close", "cert", "steady")


def test_every_combination_of_the_eight_switches():
    from pedp_hip import _lib

    assert len(_lib.ICP_SWITCHES) == 8
    seen = set()
    for bits in itertools.product((False, True), repeat=8):
        on = [n for n, b in zip(_lib.ICP_SWITCHES, bits) if b]
        p = check(on, **ELIGIBLE)
        assert p["fused"] and not p["exchange"] and p["steady_from"] == 5
        seen.add(tuple(sorted(p.items())))
    # the default process: everything on; and PEDP_NN_F32 decides nothing here
    d = check(DEFAULT, **ELIGIBLE)
    assert d["dev_result"] and d["head"] and d["certify"] and d["plan"] and d["steady"]
    assert not (d["copy_bracket"] or d["serial_close"] or d["unfused_finish"])
    assert check(DEFAULT + ("nn_f32",), **ELIGIBLE) == d
    assert len(seen) > 20
    # literal rows: one switch moved from the default at a time
    lit = lambda on: {k for k, v in check(on, **ELIGIBLE).items() if v is True}
    everything = {"fused", "dev_result", "head", "certify", "plan", "steady"}
    assert lit(DEFAULT) == everything
    assert lit(DEFAULT + ("unfused_finish",)) == {"fused", "plan", "unfused_finish"}
    assert lit(DEFAULT + ("no_visit_plan",)) == everything - {"plan"}
    assert lit(DEFAULT + ("serial_close",)) == {"fused", "dev_result", "certify", "plan", "serial_close"}
    assert lit(DEFAULT + ("copy_bracket",)) == {"fused", "copy_bracket", "certify", "plan"}
    assert lit(("cert", "steady")) == {"fused", "dev_result", "certify", "plan"}            # PEDP_ICP_HEAD_CLOSE=0
    assert lit(("head_close", "steady")) == {"fused", "dev_result", "head", "plan"}         # PEDP_ICP_CERT=0
    assert lit(("head_close", "cert")) == everything - {"steady"}                           # PEDP_ICP_STEADY=0
    # the two switches of tests/test_icp_serial_path_gpu.py
    p = check(DEFAULT + ("serial_close", "copy_bracket"), **ELIGIBLE)
    assert p["certify"] and p["plan"] and not (p["dev_result"] or p["head"] or p["steady"])


def test_exchange_batches_and_timing():
    p = check(DEFAULT, **dict(ELIGIBLE, exchange=True))
    assert p["fused"] and p["exchange"] and p["plan"] and not (p["dev_result"] or p["head"] or p["certify"] or p["steady"])
    p = check(DEFAULT, **dict(ELIGIBLE, poses=4, batch=True))
    assert p["fused"] and not (p["plan"] or p["certify"] or p["steady"] or p["dev_result"] or p["head"])
    p = check(DEFAULT, **dict(ELIGIBLE, poses=4))
    assert not (p["plan"] or p["certify"] or p["steady"])
    # a batch of one pose runs the single-pose kernel with its plan and certificates; its state still moves by the batch's kernels
    p = check(DEFAULT, **dict(ELIGIBLE, poses=1, batch=True))
    assert p["plan"] and p["certify"] and not (p["dev_result"] or p["head"] or p["steady"])
    for timed, steady in ((-1, True), (-3, True), (-2, False), (3, False)):
        p = check(DEFAULT, **dict(ELIGIBLE, timed_pass=timed))
        assert p["steady"] == steady and p["head"] and p["certify"]
    for off in ("early_exit", "no_steady"):
        p = check(DEFAULT, **dict(ELIGIBLE, **{off: True}))
        assert not p["steady"] and p["head"] and p["certify"]
    p = check(DEFAULT, **dict(ELIGIBLE, resident=False))
    assert not p["steady"] and p["head"] and p["certify"]


@pytest.mark.parametrize("change", [dict(unit_size=4), dict(exhaustive=True, unit_size=4), dict(exhaustive=True), dict(radius=0.0),
                                    dict(radius=-1.0), dict(n_target=BK_WCAP * 1024 + 1), dict(n_source=0), dict(n_target=0)])
def test_not_fused_switches_everything_below_it_off(change):
    for on in (DEFAULT, DEFAULT + ("copy_bracket", "serial_close", "unfused_finish")):
        p = check(on, **dict(ELIGIBLE, **change))
        assert not any(p[k] for k in ("fused", "dev_result", "head", "certify", "plan", "serial_close", "unfused_finish", "steady"))
        assert p["copy_bracket"] == ("copy_bracket" in on)   # (the segmented path is bracketed the same way)
    assert check(DEFAULT, **dict(ELIGIBLE, n_target=BK_WCAP * 1024))["fused"]


def test_steady_from_has_a_floor_of_one():
    for given, first in ((0, 1), (1, 1), (7, 7), (-3, 1)):
        assert check(DEFAULT, steady_from=given, **ELIGIBLE)["steady_from"] == first


def test_the_process_reads_its_switches_once_with_their_defaults_and_parsing():
    """switches=None asks for what the process read from its environment: unset switches at their defaults, a flag on
    when its value is a number other than 0 (an empty value is 0), PEDP_ICP_STEADY_FROM with its floor."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, sys.argv[1]); from pedp_hip import _lib; "
            "print(json.dumps(_lib.icp_path(None, **json.loads(sys.argv[2]))))")
    clean = {k: v for k, v in os.environ.items() if not (k.startswith("PEDP_ICP_") or k == "PEDP_NN_F32")}
    for extra, on, first in (({}, DEFAULT, 5),
                             ({"PEDP_ICP_SERIAL_CLOSE": "1", "PEDP_ICP_COPY_BRACKET": "2", "PEDP_ICP_CERT": "0", "PEDP_ICP_HEAD_CLOSE": "",
                               "PEDP_ICP_NO_VISIT_PLAN": "0", "PEDP_ICP_STEADY_FROM": "0"}, ("serial_close", "copy_bracket", "steady"), 0)):
        p = subprocess.run([sys.executable, "-c", code, root, json.dumps(ELIGIBLE)], env=dict(clean, **extra), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, p.stdout.decode()
        assert json.loads(p.stdout.decode().strip().splitlines()[-1]) == expected(on, steady_from=first, **ELIGIBLE), extra
