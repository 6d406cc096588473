"""xfh_mlpnp_solve_device (k_mlpnp_prepare / _fit / _count / _records / _refine / _decide) against the rule form of tests/ref_mlpnp.py on the scenes
and with the guarded runs of tests/mlpnp_rig.py: the header as integers, every flag and d_assigned_out equal, Tcw within one float32 step (the
device's fp64 add, mul, div and sqrt are IEEE and the library is built without contraction; sin, cos, acos and cbrt differ from the host's in last
bits, and tests/test_mlpnp_ref.py shows that no decision of these scenes hangs on them).  Shapes: n = 70 with N = 41 (a partial wave), n = 300
with N = 261 (a second 256-lane pass, a fifth 64-lane pass of the count), N = 10 / 9 / 5, iterations 1, 5, 35 and 70 (one workgroup of the fit
is 16 iterations, one of the count 4), Refine sets of 11, 64, 65 and 257 inliers, B = 1 and B = 3 with shared and per-problem draws."""
import numpy as np
import pytest

import mlpnp_rig as G
import ref_mlpnp as R
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = G.MlpnpRig(gpu_lib)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes():
    """the rig's scenes and the rule's answer for each: computed once, never changed"""
    s = G.rig()
    return s, {k: G.rule_of(v) for k, v in s.items()}


def test_every_scene_of_the_rig_equals_the_rule(rig, scenes):
    """every status and branch; what a call must leave alone still holds the bytes it held before"""
    s, want = scenes
    seen, its, planar = set(), set(), {}
    for name, sc in s.items():
        got, _ = rig.run(sc)
        planar[name] = int(got["header"][0, 10])
        print(name, dict(zip(R.HEADER, got["header"][0].tolist())))
        G.assert_equals_rule(got, want[name], 0, prior_byte=0xA5)
        assert R.STATUS[got["header"][0, 1]] == G.EXPECT[name], name
        seen.add(int(got["header"][0, 1])); its.add(int(got["header"][0, 2]))
    assert seen == {0, 1, 2, 3} and {1, 5, 35, 70} <= its
    assert planar["planar"] == 1 and planar["n70"] == 0                                                        # the planar branch was taken
    for name, size in G.REFINE_SETS.items():
        assert want[name]["counts"][want[name]["header"][6]] == size


def test_three_candidates_against_separate_calls_and_two_runs(rig):
    fam = G.family()
    got, raw = rig.run(fam)
    for b, st in enumerate((R.REFINED, R.NONE, R.TOO_FEW)):
        G.assert_equals_rule(got, G.rule_of(fam, b), b, prior_byte=0xA5)
        assert got["header"][b, 1] == st
    assert np.array_equal(rig.run(fam)[1], raw)                              # two runs give identical bytes
    lay3, lay1 = Context.mlpnp_layout(3, 70, G.GUARD), Context.mlpnp_layout(1, 70, G.GUARD)
    for b in range(3):
        one = dict(fam, assigned=fam["assigned"][b:b + 1], points=fam["points"][b:b + 1], valid=fam["valid"][b:b + 1], draws=fam["draws"][b:b + 1])
        _, raw1 = rig.run(one)
        for k in Context.MLPNP_OUT:
            per = lay1[k + "_bytes"]
            assert np.array_equal(raw1[lay1[k]:lay1[k] + per], raw[lay3[k] + b * per:lay3[k] + (b + 1) * per]), (b, k)


def test_shared_draws_equal_per_problem_copies(rig):
    fam = G.family()
    d = fam["draws"][0]
    got, raw = rig.run(fam, draws=d)                                         # stride 0
    assert np.array_equal(rig.run(fam, draws=np.stack([d, d, d]))[1], raw)
    for b in range(3):
        G.assert_equals_rule(got, G.rule_of(dict(fam, draws=np.stack([d, d, d])), b), b, prior_byte=0xA5)


def test_resumed_calls_equal_the_rule(rig, scenes):
    """d_start_iter = the previous header's consumed count, per problem; and a start past the draws"""
    s, want = scenes
    for name in ("n70", "its70", "n_equals_min"):
        sc, start, cache = s[name], 0, {}
        for call in range(3):
            w = G.rule_of(sc, start_iter=start, cache=cache)
            got, _ = rig.run(sc, start_iter=[start])
            G.assert_equals_rule(got, w, 0, prior_byte=0xA5)
            if w["header"][1] != R.REFINED:
                break
            start = int(w["header"][8])
        assert call > 0 or name == "n_equals_min"
    for start in (34, 35, 10 ** 9, -4):
        got, _ = rig.run(s["n70"], start_iter=[start])
        G.assert_equals_rule(got, G.rule_of(s["n70"], start_iter=start), 0, prior_byte=0xA5)
    fam = G.family()
    starts = [3, 0, 0]
    got, _ = rig.run(fam, start_iter=starts)
    for b in range(3):
        G.assert_equals_rule(got, G.rule_of(fam, b, start_iter=starts[b]), b, prior_byte=0xA5)


def test_chunk_lengths_and_the_optional_valid_array(rig, scenes):
    s, _ = scenes
    for chunk in (0, 1, 20):
        sc = dict(s["n_equals_min"], chunk=chunk, draws=np.repeat(s["n_equals_min"]["draws"], 4, axis=1))
        G.assert_equals_rule(rig.run(sc)[0], G.rule_of(sc), 0, prior_byte=0xA5)
    sc = s["n70"]
    got, _ = rig.run(sc, valid=False)                                        # NULL: every point is valid, three more correspondences
    w = G.rule_of(sc, point_valid=None)
    assert w["header"][0] == 44
    G.assert_equals_rule(got, w, 0, prior_byte=0xA5)


def test_gating_by_the_bow_match_count(rig, scenes):
    s, want = scenes
    got, _ = rig.run(s["n70"], n_matches=[14], min_matches=15)
    G.assert_equals_rule(got, G.rule_of(s["n70"], n_matches=14, min_matches=15), 0, prior_byte=0xA5)
    assert got["header"][0, 1] == R.TOO_FEW
    got, _ = rig.run(s["n70"], n_matches=[15], min_matches=15)
    G.assert_equals_rule(got, want["n70"], 0, prior_byte=0xA5)


def test_hostile_input_returns_meets_the_rule_and_keeps_the_guards(rig):
    """indices of +-2^31, draws out of range, NaN and Inf points and keypoints; then tables of INT_MAX / INT_MIN / 0"""
    sc = G.hostile()
    G.assert_equals_rule(rig.run(sc)[0], G.rule_of(sc), 0, prior_byte=0xA5)
    n = sc["assigned"].shape[1]
    for ti, tm in ((2 ** 31 - 1, 0), (-2 ** 31, -2 ** 31), (0, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        tables = (np.full(n + 1, ti, np.int64).astype(np.int32), np.full(n + 1, tm, np.int64).astype(np.int32))
        got, _ = rig.run(sc, tables=tables)
        G.assert_equals_rule(got, G.rule_of(dict(sc, tables=tables)), 0, prior_byte=0xA5)
