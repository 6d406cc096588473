"""The two restatements of SearchForInitialization (tests/ref_init.py: the literal loop and the order-free rule the device resolves) against
each other on the seeded scenes and on random small ones, xfh_init_accept on every boundary, hand-made cases whose answers are written out,
the refusals of both entry points with a NULL ctx, kernel names and ids, the header helper under AddressSanitizer + UBSan as a stand-alone
program, and the conditions of the seeded scenes the GPU test uses (the frames come from the CPU oracle's extraction here: this is where
the seeds are chosen).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import init_rig as IR
import ref_init as RI
import ref_window as RW
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = RI.NONE
SCENES = [(1200, 1000), (1201, 4096)]                                 # (image seed, nfeatures) of the GPU test
WINDOW = 100.0                                                        # Tracking.cc:2519
DEPTH_MIN = RI.DEPTH_MIN                                              # what the GPU test may expect of the resolver's round count
BOUNDS = (0.0, 0.0, 640.0, 480.0)


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as g
    if not os.path.exists(capi.LIB_PATH):
        g.build()


def test_accept_line_on_every_boundary():
    acc = Context.init_accept
    assert acc(100, NONE, 100, 0.9) and not acc(101, NONE, 100, 0.9)                          # best == th_low, th_low + 1
    assert acc(0, NONE, 100, 0.9) and acc(100, NONE, 100, 1e-7)                               # second == INT_MAX: 2^31 as a float
    assert not acc(100, NONE, 100, 0.0) and not acc(0, 0, 100, 0.9)
    assert acc(49, 100, 100, 0.5) and not acc(50, 100, 100, 0.5) and not acc(51, 100, 100, 0.5)   # best == second * nn_ratio exactly: strict '<'
    assert acc(89, 100, 100, 0.9) == bool(F(89) < F(100) * F(0.9)) and acc(90, 100, 100, 0.9) == bool(F(90) < F(100) * F(0.9))
    assert not acc(NONE, NONE, NONE, 2.0)                                                      # nothing tested
    rng = np.random.RandomState(3)
    for _ in range(2000):
        b, s, t = (int(v) for v in rng.randint(0, 300, 3))
        r = float(F(rng.rand()))
        assert acc(b, s, t, r) == RI.accept(b, s, t, r), (b, s, t, r)


def test_refusals_with_a_null_ctx_kernel_names_and_layout():
    L = capi.lib()
    p = C.c_void_p(4096)
    gb = capi.GridBounds(*BOUNDS)
    assert L.xfh_init_search_device(None, 1, 8, p, p, None, 100.0, p, p, 0, None, 8, 100, 0.9, p, p, p, p, p, p, p, p, p, p, p, None) == 1
    assert L.xfh_init_search(None, 8, p, p, None, 100.0, p, C.byref(gb), p, 8, 100, 0.9, p, p, p, p, p, p, p, p, p, p, None) == 1
    K = capi.K
    assert (K["INIT_CANDIDATES"], K["INIT_RESOLVE"], K["INIT_FINAL"]) == (27, 28, 29)
    assert [L.xfh_kernel_name(i) for i in (26, 27, 28, 29, 30)] == [b"?", b"k_init_candidates", b"k_init_resolve", b"k_init_final", b"?"]
    assert L.xfh_kernel_name(25) == b"k_sim3_agree" and L.xfh_kernel_name(17) == b"k_proj_resolve"      # existing ids keep their values
    assert (capi.INIT_INACTIVE, capi.INIT_NO_CANDIDATES, capi.INIT_REJECTED, capi.INIT_MATCHED) == (RI.INACTIVE, RI.NO_CANDIDATES, RI.REJECTED, RI.MATCHED)
    lay = Context.init_search_layout(2, 100, 50, 256)
    assert 2 <= lay["K"] <= 16 and lay["K"] == L.xfh_init_list_entries()
    assert Context.init_search_workspace_bytes(100, 50, 2) == 2 * Context.init_search_workspace_bytes(100, 50, 1) > 0
    assert all(Context.init_search_workspace_bytes(*a) == 0 for a in ((0, 8, 1), (8, 0, 1), (capi.GRID_MAX_N + 1, 8, 1), (8, capi.GRID_MAX_N + 1, 1), (8, 8, 0), (8, 8, 65536)))


def test_header_helper_under_sanitizers(tmp_path):
    """xfh_init_accept against init_math.h compiled into the program, the layout helper and the NULL-ctx refusals: a stand-alone program built
    with AddressSanitizer + UBSan against the sanitizer build of the HOST code (make -C xfeatslam_amd/csrc asan; device code is not
    instrumented, nothing runs on a GPU, nothing is loaded into Python)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "asan", "-s", "-j8"])
    exe = str(tmp_path / "asan_init_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_init_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip_asan", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_init_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ---- hand-made cases: rows are multiples of unit vectors, so every distance is 512 * (difference)^2 and can be read off -------------------
def row(j, s):
    e = np.zeros(64, F); e[j] = s
    return e


def at(d):
    return float(np.sqrt((d + 0.25) / 512.0))


def handmade():
    """(name, queries [(x, y, row)], targets [(x, y, row)], window, flags, wanted outputs)"""
    T = [(100.0, 100.0, row(0, 0.0)), (130.0, 100.0, row(1, 1.0))]    # T1 is 512 + from every query on axis 0
    M, R, N = RI.MATCHED, RI.REJECTED, RI.NO_CANDIDATES
    return [
        # Q0 takes T0 at 50; Q1 is strictly closer, takes it away, and Q0 stays without a match although T1 was in its window
        ("retraction", [(100, 100, row(0, at(50))), (100, 100, row(0, at(10)))], T, 50.0, None,
         dict(status=[M, M], claim_idx=[0, 0], matches12=[-1, 0], best_dist=[50, 10], n_window=[2, 2], n_tested=[2, 2], matches21=[1, -1], matched_distance=[10, NONE],
              n_matches=1)),
        # the later query is farther: T0 is blocked, its best is T1 at 512 + 50: rejected, and the earlier match stays
        ("blocked", [(100, 100, row(0, at(10))), (100, 100, row(0, at(50)))], T, 50.0, None,
         dict(status=[M, R], claim_idx=[0, -1], matches12=[0, -1], best_dist=[10, 562], second_dist=[522, NONE], n_tested=[2, 1], matches21=[0, -1],
              matched_distance=[10, NONE], n_matches=1)),
        # an equal distance is blocked ('<=')
        ("equal", [(100, 100, row(0, at(10))), (100, 100, row(0, at(10)))], T, 20.0, None,
         dict(status=[M, R], claim_idx=[0, -1], matches12=[0, -1], best_dist=[10, NONE], second_dist=[NONE, NONE], n_window=[1, 1], n_tested=[1, 0], n_matches=1)),
        # all members blocked: REJECTED with n_tested == 0; and an empty window
        ("all blocked, empty", [(100, 100, row(0, 0.0)), (100, 100, row(0, at(5))), (400, 300, row(0, 0.0))], T, 20.0, None,
         dict(status=[M, R, N], claim_idx=[0, -1, -1], best_dist=[0, NONE, NONE], n_window=[1, 1, 0], n_tested=[1, 0, 0], matches21=[0, -1], n_matches=1)),
        # an inactive query in between changes nothing; flags clear -> INACTIVE with zeros
        ("inactive", [(100, 100, row(0, at(50))), (100, 100, row(0, at(10))), (100, 100, row(0, at(5)))], T, 50.0, [1, 0, 1],
         dict(status=[M, RI.INACTIVE, M], claim_idx=[0, -1, 0], matches12=[-1, -1, 0], best_dist=[50, NONE, 5], n_window=[2, 0, 2], n_tested=[2, 0, 2], matches21=[2, -1],
              matched_distance=[5, NONE], n_matches=1)),
        # the ratio test fails on a free second best and passes once that one is held (T1 moved next to T0 in descriptor space)
        ("ratio flip", [(100, 100, row(0, at(20) + at(21))), (100, 100, row(0, at(20)))], [(100.0, 100.0, row(0, 0.0)), (130.0, 100.0, row(0, at(20) + at(21)))], 50.0, None,
         dict(status=[M, M], claim_idx=[1, 0], matches12=[1, 0], best_dist=[0, 20], second_dist=[82, NONE], n_tested=[2, 1], matches21=[1, 0], matched_distance=[20, 0],
              n_matches=2)),
        # above th_low: rejected although alone
        ("th_low", [(100, 100, row(0, at(101))), (100, 100, row(0, at(100)))], T[:1], 50.0, None,
         dict(status=[R, M], best_dist=[101, 100], n_tested=[1, 1], matches12=[-1, 0], n_matches=1)),
    ]


def run_case(O, form, queries, targets, window, flags):
    tx = np.array([t[0] for t in targets], F); ty = np.array([t[1] for t in targets], F)
    tg = np.stack([t[2] for t in targets]).astype(F)
    q = np.stack([c[2] for c in queries]).astype(F)
    pm = np.array([[c[0], c[1]] for c in queries], F)
    grid = RW.build(tx, ty, BOUNDS)
    return form(O, q, pm, window, grid, tx, ty, BOUNDS, tg, flags=None if flags is None else np.array(flags, np.uint8), txy=np.stack([tx, ty], 1))


def test_hand_made_cases(oracle_mod):
    cases = handmade()
    assert len(cases) == 7
    for name, queries, targets, window, flags, want in cases:
        for form in (RI.literal, RI.order_free):
            m = run_case(oracle_mod, form, queries, targets, window, flags)
            for key, val in want.items():
                got = m[key] if np.isscalar(m[key]) else m[key].tolist()
                assert got == val, (name, form.__name__, key, got, val)
            # the update of vbPrevMatched: the matched keypoint's coordinates, the old centre otherwise
            for i, c in enumerate(queries):
                k = m["matches12"][i]
                assert m["prev_out"][i].tolist() == ([targets[k][0], targets[k][1]] if k >= 0 else [float(c[0]), float(c[1])]), (name, i)


def test_the_two_forms_agree_on_random_small_scenes(oracle_mod):
    """overlapping windows, few distinct rows (so distances repeat and ties and equalities occur), some inactive queries"""
    for seed in range(30):
        rng = np.random.RandomState(seed)
        nq, nt = int(rng.randint(20, 120)), int(rng.randint(5, 80))
        tx = rng.uniform(200, 330, nt).astype(F); ty = rng.uniform(150, 260, nt).astype(F)
        protos = (rng.randn(6, 64) * 0.05).astype(F)
        tg = (protos[rng.randint(6, size=nt)] + (rng.randn(nt, 64) * 0.004).astype(F) * (rng.rand(nt, 1) < 0.7)).astype(F)
        q = (protos[rng.randint(6, size=nq)] + (rng.randn(nq, 64) * 0.012).astype(F) * (rng.rand(nq, 1) < 0.8)).astype(F)
        pm = np.stack([rng.uniform(180, 350, nq), rng.uniform(130, 280, nq)], 1).astype(F)
        flags = (rng.rand(nq) < 0.9).astype(np.uint8) if seed % 3 == 0 else None
        grid = RW.build(tx, ty, BOUNDS)
        kw = dict(flags=flags, th_low=int(rng.choice([30, 100, 400])), nn_ratio=float(rng.choice([0.6, 0.9, 1.0])), txy=np.stack([tx, ty], 1))
        a = RI.literal(oracle_mod, q, pm, float(rng.choice([40.0, 100.0])), grid, tx, ty, BOUNDS, tg, **kw)
        b = RI.order_free(oracle_mod, q, pm, 0.0, grid, tx, ty, BOUNDS, tg, members=a["members"], **kw)
        assert RI.same(a, b) == [], (seed, RI.same(a, b))
        assert a["n_matches"] == int((a["matches12"] >= 0).sum()) == int((a["matches21"] >= 0).sum())


@pytest.fixture(scope="module")
def scenes(oracle_mod, weights_dense):
    out = {}
    K = Context.init_search_layout(1, 8, 8)["K"]
    for seed, nf in SCENES:
        fr, bounds = IR.cpu_frames(oracle_mod, weights_dense[1], nf, seed)
        q, pm, tg, info = RI.plant(seed, fr[0][0], fr[0][1], fr[1][0], fr[1][1], K)
        x, y = fr[1][0][:, 0].copy(), fr[1][0][:, 1].copy()
        out[seed] = dict(q=q, pm=pm, tg=tg, info=info, x=x, y=y, bounds=bounds, grid=RW.build(x, y, bounds), txy=fr[1][0], valid=fr[0][2], K=K)
    return out


@pytest.mark.parametrize("seed,nf", SCENES)
def test_seeded_scenes_show_what_the_order_exists_for(oracle_mod, scenes, seed, nf):
    """what tests/init_rig.py builds on the device, from the CPU oracle's extraction: problem 0 of the GPU test at window = 100.  The two forms
    agree on it, and the literal form shows: a retraction, an answer that differs from the search with no blocking, a ratio test that flips
    because its second best was blocked, an acceptor chain of at least 8 on one keypoint, a dependence depth of at least DEPTH_MIN, and a
    query with more than K blocked members ahead of its answer (K from the library)."""
    s = scenes[seed]
    args = (oracle_mod, s["q"], s["pm"], WINDOW, s["grid"], s["x"], s["y"], s["bounds"], s["tg"])
    seq = RI.literal(*args, txy=s["txy"])
    free = RI.literal(*args, txy=s["txy"], blocking=False, members=seq["members"])
    of = RI.order_free(*args, txy=s["txy"], members=seq["members"])
    assert RI.same(seq, of) == [], RI.same(seq, of)
    c = RI.conditions(seq, free, of["depth"], s["K"])
    print(f"seed {seed} nf {nf} K {s['K']}: statuses {np.bincount(seq['status'], minlength=4).tolist()}, valid queries {int(s['valid'].sum())}, "
          f"mean window {float(seq['n_window'].mean()):.0f}, {c}")
    assert c["retractions"] >= 1 and c["differs"] >= 1 and c["flips"] >= 1 and c["chain"] >= 8 and c["depth"] >= DEPTH_MIN and c["ran_out"] >= 1, c
    assert c["n_matches"] >= nf // 8
    # the planted structures did what they were planted for
    info = s["info"]
    assert int((seq["claim_idx"] == info["run_target"]).sum()) >= 12
    st, T = info["stairs"]
    assert [int(seq["claim_idx"][q]) for q in st] == T and [int(free["claim_idx"][q]) for q in st[1:]] == T[:-1]
    tw, V = info["twins"]
    assert seq["claim_idx"][tw[0]] == V and seq["claim_idx"][tw[1]] != V and free["claim_idx"][tw[1]] == V
    hold, P = info["pile"]
    assert seq["blocked_ahead"][hold[-1]] >= s["K"] + 4
    fl, (Wa, Wb) = info["flip"]
    assert seq["flips"][fl[1]] and seq["claim_idx"][fl[1]] == Wa and free["status"][fl[1]] == RI.REJECTED
