"""Host half of the Schur referee (tests/test_gpu_schur_referee.py): on the CPU, without a device,

  * the numpy statement of the reduction (tests/schur_statement.py) and the fp64 oracle agree with the long-double oracle in the
    entrywise scale on every window of tests/schur_cases.py — their larger deviation is e_ref, the yardstick of the GPU bound;
  * five wrong reductions — the last landmark of a ragged stage left out, one (landmark, block) pair left out, one landmark's
    V^-1 b left out of the right-hand side, the landmark damping omitted under LM, one off-diagonal block transposed — each exceed
    BOUND_FACTOR x e_ref at least tenfold on every window they apply to, so a kernel that made one of them would fail the GPU test;
  * the windows have the shapes the kernels' paths need, asserted from pairs() and the index lists: a landmark with a single
    block, a stage of four landmarks with a missing pair, a ragged last stage, chunks beyond one batch of 12 and of 16 landmarks,
    a landmark without a pair in one tile of an off-diagonal tile pair, pose parts of 18 / 60 / 66 / 96 / 102 / 198 rows.

Measured (profiles/schur_referee_notes.md), unweighted scale: e_ref REDUCED_S 1.18e-6 over the whole array (pose x speed/bias
entries of the IMU factors, none of the reduction's), 1.49e-8 over the pose part, 2.37e-14 over the landmark-only entries (fp64
against long double on identical inputs); REDUCED_RHS 1.17e-7.  Smallest mutation / bound: 11.9 (whole array), 76.5 (pose part)."""
import numpy as np
import pytest

from okvis_amd import solver

from . import schur_cases as cases
from . import schur_statement as stmt


@pytest.fixture(scope="module")
def ref(oracle):
    assert np.finfo(np.longdouble).eps < 2e-19, "the referee needs an extended long double"
    r = cases.Referee(oracle)
    for a in cases.ARRAYS:
        print(f"SCHURREF e_ref {a} whole array {r.e_ref[a][0]:.3e} pose part {r.e_ref[a][1]:.3e} "
              f"(scale {'weighted with cond(Vd)' if cases.WEIGHTED else 'unweighted'})")
    print(f"SCHURREF e_ref REDUCED_S landmark-only entries {r.e_ref_landmark_only:.3e}")
    return r


def _each(ref):
    for (name, kind), solved in ref.solved.items():
        for i, s in enumerate(solved):
            yield name, kind, i, s


def test_statement_and_oracle_agree_with_the_extended_referee(ref):
    for name, kind, i, s in _each(ref):
        for a in cases.ARRAYS:
            print(f"SCHURREF host {name} {kind} w{i} {a} whole array: e_oracle {s.e_oracle[a][0]:.3e} e_stmt {s.e_stmt[a][0]:.3e} | "
                  f"pose part: e_oracle {s.e_oracle[a][1]:.3e} e_stmt {s.e_stmt[a][1]:.3e} | "
                  f"other scale ({'un' if cases.WEIGHTED else ''}weighted), whole array: e_oracle {s.e_oracle_other[a]:.3e}")
            for p in (0, 1):
                assert s.e_stmt[a][p] <= ref.e_ref[a][p] and s.e_oracle[a][p] <= ref.e_ref[a][p]
        print(f"SCHURREF host {name} {kind} w{i} STEP e_oracle {s.e_step:.3e} | landmark-only entries of S: {int(s.landmark_only.sum())}, "
              f"fp64 against long double on the same inputs {s.e_landmark_only:.3e}")
        assert s.landmark_only.any() and 0.0 < s.e_landmark_only <= ref.e_ref_landmark_only
        S = s.ref["REDUCED_S"]
        assert np.abs(S - S.T).max() <= 1e-15 * np.abs(S).max()
    # a yardstick of rounding size: far below what a wrong reduction does, not nothing
    for a in cases.ARRAYS:
        for p in (0, 1):
            assert 1e-17 < ref.e_ref[a][p] < 1e-5, (a, p, ref.e_ref[a])
        assert ref.e_ref[a][1] <= ref.e_ref[a][0]
    assert 1e-17 < ref.e_ref_landmark_only < 1e-12, ref.e_ref_landmark_only


@pytest.mark.parametrize("mutation", stmt.MUTATIONS)
def test_a_wrong_reduction_exceeds_the_bound_tenfold(ref, mutation):
    array = "REDUCED_RHS" if mutation == "drop_vb" else "REDUCED_S"
    seen = 0
    for name, kind, i, s in _each(ref):
        if mutation == "no_lm_damping" and kind != "lm":
            continue
        if mutation == "ragged_last":
            assert ref.windows[name][i].n_lm % 4 != 0, name
        S, rhs = s.statement(s.o64, np.float64, mutate=mutation)
        got = dict(REDUCED_S=S, REDUCED_RHS=rhs)[array]
        for p in (False, True):      # against the whole array's bound with the whole array's deviation, and the pose part's with its own
            e = s.deviation(array, got, p)
            print(f"SCHURREF mutation {mutation} {name} {kind} w{i} {array} {'pose part' if p else 'whole array'} {e:.3e} = "
                  f"{e / ref.bound(array, p):.1f} x bound")
            assert e >= cases.MUTATION_MARGIN * ref.bound(array, p), (mutation, name, kind, i, p, e, ref.bound(array, p))
        # the landmark-only entries against the statement in long double: every left-out landmark and the missing damping show there
        e = s.deviation_landmark_only(S, s.statement(s.o64, np.longdouble)[0])
        print(f"SCHURREF mutation {mutation} {name} {kind} w{i} REDUCED_S landmark-only {e:.3e} = "
              f"{e / (cases.BOUND_FACTOR * ref.e_ref_landmark_only):.1e} x bound")
        if mutation in ("ragged_last", "no_lm_damping"):
            assert e >= cases.MUTATION_MARGIN * cases.BOUND_FACTOR * ref.e_ref_landmark_only, (mutation, name, kind, i, e)
        seen += 1
    assert seen >= 5


def _stages(lists):
    """(pairs in the stage, landmarks in the stage, chunk) of every stage of four landmarks"""
    first = np.asarray(lists["lm_pair_begin"])
    for c, (lb, le) in enumerate(cases.chunk_landmarks(lists)):
        for l0 in range(lb, le, 4):
            l1 = min(l0 + 4, le)
            yield int(first[l1] - first[l0]), l1 - l0, c


def test_the_windows_have_the_shapes_the_kernels_paths_need(ref):
    Dps = set()
    for name, (_, kinds, upload) in cases.CASES.items():
        for i, w in enumerate(ref.windows[name]):
            s = ref.solved[name, kinds[0]][i]
            Dps.add(s.Dp if name in cases.SMALL + cases.LARGE else -1)
            pair_lm, pair_block = s.pairs
            per_lm = np.bincount(pair_lm, minlength=w.n_lm)
            nblk = s.Dp // 6
            assert (per_lm == 1).any() or name.startswith("ext_"), name          # a landmark seen by a single pose block
            assert per_lm.min() >= 1
            lists = solver.index_lists(w, ref.options(name, "dogleg", reserved0=4), len(ref.windows[name]))
            stages = list(_stages(lists))
            assert any(n < nl * nblk for n, nl, _ in stages), name                # a stage with a missing pair
            assert any(nl < 4 for _, nl, _ in stages), name                       # a ragged last stage
            sizes = [le - lb for lb, le in cases.chunk_landmarks(lists)]
            assert sum(sizes) == w.n_lm and max(sizes) <= 64
            if "wide" in name:
                # several chunks, one beyond a batch of 12 and of 16 landmarks, one that ends in a ragged batch and a ragged stage
                assert len(sizes) >= 2 and max(sizes) > 16 and any(n % 12 and n % 16 and n % 4 for n in sizes), (name, sizes)
            print(f"SCHURREF shapes {name} w{i} Dp {s.Dp} chunks {sizes}")
            if name in cases.TILED:
                tile = pair_block // 16      # fixed extrinsics: block index = pose index = reduced block
                assert np.array_equal(s.off[pair_block], 6 * pair_block)
                in0 = np.bincount(pair_lm[tile == 0], minlength=w.n_lm) > 0
                in1 = np.bincount(pair_lm[tile == 1], minlength=w.n_lm) > 0
                assert (in0 & ~in1).any() and (in0 & in1).any(), name             # tile pair (1, 0): a landmark absent from one side
    assert {18, 60, 66, 96, 102, 198} <= Dps, Dps
    assert [s.Dp for s in ref.solved["ragged", "dl"]] == [18, 42, 60]
