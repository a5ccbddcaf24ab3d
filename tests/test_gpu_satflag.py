"""dq-init + saturation flagging on the device (misc.hip: sat_exceed_kernel / sat_flags_kernel, in front of rip_calibrate) against
the numpy restatement oracle/saturation.py on the planted cases of satflag_cases.py (test_host_satflag_cases.py holds the cases
and the restatement to two further statements of the rule without a GPU).

Every call is a ramp-fit-only call (stages=STAGE_RAMPFIT): it has no 128-column rule, and the stage ramp fit takes 2 to 64
groups.  Per case and backup two calls are made in one CALDIR slot: one that flags on the device, one that is handed the flags the
restatement made.  Every output of the two must be the same bit for bit, and the saturation bits of the first are compared with the
restatement's directly.  No tolerance anywhere.  Each test prints the counts of flagged groups and pixels and of differing words.

Held by these cases, each of which fails on the kernels as they were before:
  * a +inf sample of an f32 cube at a pixel that is not checked (NaN or infinite threshold, NO_SAT_CHECK) raises no flag, with
    and without the read-pattern rule (samples_f32, samples_f32_rule);
  * thresholds between 3.4e38 and FLT_MAX are checked, as np.isfinite has it (thresholds_f32);
and, defined behaviour now: skip_firstn == 64 (pos_16x16_g64_skip64) and a backup far above the group count (10**9)."""

import numpy as np
import pytest
import torch  # noqa: F401  before libromanhip is loaded: the first HIP runtime loaded must be the one both use
from chain_support import assert_equal_outputs, chain_context, loaded
from conftest import assert_same_bits

import satflag_cases as sc
from romanimpreprocess_amd import pipeline, synth

pytestmark = pytest.mark.gpu

SAT = sc.SAT
SLOT = 9


def _cal(c, with_saturation=True):
    cal = dict(synth.make_caldir(c.ny, c.nx, read_pattern=c.rp, p_order=3, seed=300 + c.G, nb=4, with_biascorr=False))
    cal["saturation"] = {"data": c.thr, "dq": c.sdq}
    if not with_saturation:
        del cal["saturation"]
    return cal


def _ramp(c, groupdq, pixeldq):
    return {"data": c.data, "groupdq": groupdq, "pixeldq": pixeldq, "read_pattern": c.rp, "frame_time": synth.FRAME_TIME}


def _on_device(cb, c, backup, groupdq="case", skip=None):
    """the call that flags on the device"""
    given = c.groupdq if isinstance(groupdq, str) else groupdq
    return cb.calibrate(SLOT, _ramp(c, given, c.pixeldq), stages=pipeline.STAGE_RAMPFIT, exclude_first=c.exclude_first,
                        flag_saturation=True, saturation_backup=backup, saturation_skip_firstn=c.skip if skip is None else skip,
                        saturation_read_pattern=c.rule)


def _handed(cb, c, gdq, pdq):
    """the same call on the flags the restatement made"""
    return cb.calibrate(SLOT, _ramp(c, gdq, pdq), stages=pipeline.STAGE_RAMPFIT, exclude_first=c.exclude_first)


def _compare(cb, c, backup, got=None, what=None):
    """device flags of `backup` (or the result `got` of another call that must mean the same) against the restatement's"""
    what = what or f"{c.name}, backup {backup}"
    gdq, pdq = sc.flag_host(c, min(backup, 70))     # (the restatement loops `backup` times; beyond G - 1 nothing changes)
    got = _on_device(cb, c, backup) if got is None else got
    want = _handed(cb, c, gdq, pdq)
    ndiff = int(np.count_nonzero((got["groupdq"] & SAT) != (gdq & SAT)) + np.count_nonzero((got["pixeldq"] & SAT) != (pdq & SAT)))
    print(f"{what}: {np.count_nonzero(gdq & SAT)} groups and {np.count_nonzero(pdq & SAT)} pixels flagged, "
          f"{ndiff} differing words")
    assert_same_bits(got["groupdq"] & SAT, gdq & SAT, f"{what}: SATURATED in groupdq")
    assert_same_bits(got["pixeldq"] & SAT, pdq & SAT, f"{what}: SATURATED in pixeldq")
    assert_equal_outputs(got, want, what)
    return got


@pytest.mark.parametrize("name", sc.case_names())
def test_device_flags_match_the_restatement(name):
    c = sc.case(name)
    ctx = chain_context()
    with loaded(pipeline.Calibrator(ctx=ctx), SLOT, _cal(c)) as cb:
        if not c.runs_on_device:
            # one group: no plan, hence no call (satflag_cases.py); refused by name, and the context goes on below
            with pytest.raises(ValueError, match="plan: 1 groups unsupported"):
                _on_device(cb, c, 0)
            print(f"{name}: refused by name (a plan needs 2 groups)")
            return
        outs = {}
        for backup in c.backups:
            got = outs[backup] = _compare(cb, c, backup)
            # the given bits survive
            if c.groupdq is not None:
                assert_same_bits(got["groupdq"] & c.groupdq, c.groupdq, f"{name}: given group bits")
            assert_same_bits(got["pixeldq"] & c.pixeldq, c.pixeldq, f"{name}: given pixel bits")
            assert bool(np.all((got["groupdq"][0] & sc.DNU) != 0)) == c.exclude_first
            if c.groupdq is None:   # no groupdq means a zero groupdq
                zero = _on_device(cb, c, backup, groupdq=np.zeros(c.data.shape, np.uint8))
                assert_equal_outputs(got, zero, f"{name}, backup {backup}: groupdq None vs zeros")
        # at and beyond the group count a backup says the same
        G = c.G
        if {G - 1, G, G + 6} <= set(outs):
            for backup in (G, G + 6):
                assert_equal_outputs(outs[backup], outs[G - 1], f"{name}: backup {backup} vs {G - 1}")


@pytest.mark.parametrize("name", ["pos_16x16_g2_skip0", "pos_16x16_g2_skip1"])
def test_a_backup_of_a_billion_is_a_backup_of_the_group_count(name):
    """rip_launch_satflag clamps the backup to the group count: larger values mean the same (include/romanhip.h), and no thread
    loops a billion times"""
    c = sc.case(name)
    with loaded(pipeline.Calibrator(ctx=chain_context()), SLOT, _cal(c)) as cb:
        one = _compare(cb, c, 1)
        huge = _compare(cb, c, 1, got=_on_device(cb, c, 10**9), what=f"{name}, backup 10**9")
        assert_equal_outputs(huge, one, f"{name}: backup 10**9 vs 1")


def test_refusals_leave_the_context_usable():
    c = sc.case("pos_16x20_g8_skip1")
    ctx = chain_context()
    cb = pipeline.Calibrator(ctx=ctx)
    bad = "saturation flagging: bad group / backup / skip arguments"
    with loaded(cb, SLOT, _cal(c)):
        for what, kw in (("negative backup", {"backup": -1}), ("negative skip", {"backup": 1, "skip": -1}),
                         ("skip above the group count", {"backup": 1, "skip": c.G + 1})):
            with pytest.raises(ValueError, match=bad):
                _on_device(cb, c, **kw)
            _compare(cb, c, 1, what=f"after a refusal ({what})")
    with loaded(cb, SLOT, _cal(c, with_saturation=False)):
        with pytest.raises(ValueError, match="flag_saturation needs the saturation array"):
            _on_device(cb, c, 1)
        gdq, pdq = sc.flag_host(c, 1)
        got = _handed(cb, c, gdq, pdq)     # the set still serves a call that brings its flags
        assert_same_bits(got["groupdq"] & SAT, gdq & SAT, "handed flags on a set without saturation")
    one = sc.case("pos_16x16_g1_skip0")
    with loaded(cb, SLOT, _cal(one)):
        with pytest.raises(ValueError, match="plan: 1 groups unsupported"):
            _on_device(cb, one, 0)
    with loaded(cb, SLOT, _cal(c)):
        _compare(cb, c, 2, what="after every refusal")
