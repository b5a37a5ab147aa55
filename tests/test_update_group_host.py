"""The host side of the group update: ddrl_update_group_plan (a pure function, no GPU) lays the chains
of M members x P policies out over launches of at most `cap` chains -- chain c of a launch on blocks
32 (c >> 3) + 8 j + (c & 7), j = 0 .. 3 -- and the binding carries every new symbol."""
import numpy as np
import pytest

from ddrl_amd import native as N

CAPS = (4, 7, 8, 12, 13, 24, 63, 64)


def _launches(lom, P):
    """chains of every launch"""
    return [int((lom == l).sum()) * P for l in range(int(lom[-1]) + 1)]


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_plan_layout(P):
    for cap in (c for c in CAPS if c >= P):
        for M in range(1, 65):
            lom, first = N.update_group_plan(M, P, cap)
            assert lom.shape == (M,) and first.shape == (M, P)
            # members stay whole and in order, no launch passes its cap, launches are numbered densely
            assert lom[0] == 0 and (np.diff(lom) >= 0).all() and (np.diff(lom) <= 1).all()
            chains = _launches(lom, P)
            assert all(0 < n <= cap for n in chains) and sum(chains) == M * P
            for l, n in enumerate(chains):
                rows = (n + 7) // 8
                grid = N.update_group_grid(n)
                assert grid == 32 * (rows - 1) + 24 + (n - 8 * (rows - 1))
                owner = {}
                for m in np.flatnonzero(lom == l):
                    for p in range(P):
                        blocks = [int(first[m, p]) + 8 * j for j in range(4)]
                        assert len({b % 8 for b in blocks}) == 1            # one XCD under the round robin
                        assert all(0 <= b < grid for b in blocks)
                        for b in blocks:
                            assert owner.setdefault(b, (m, p)) == (m, p)    # no block belongs to two chains
                assert len(owner) == 4 * n
                # at most 4 * ceil(n / 8) workgroups on any XCD: the residency the cap is computed from
                per_xcd = np.bincount([b % 8 for b in owner], minlength=8)
                assert per_xcd.max() <= 4 * rows


def test_plan_refusals():
    for args, why in (((0, 4, 64), "at least one member"), ((2, 0, 64), "n_policies must be"),
                      ((2, 5, 64), "n_policies must be"), ((2, 4, 3), "cannot hold a member's 4")):
        with pytest.raises(N.DdrlError, match=why):
            N.update_group_plan(*args)


def test_binding_carries_the_group_symbols():
    names = {"ddrl_update_group_create", "ddrl_update_group_run", "ddrl_update_group_finish",
             "ddrl_update_group_plan", "ddrl_update_group_placement", "ddrl_update_group_destroy"}
    assert names <= set(N.header_symbols())
    assert names <= set(N._SIGS)
    lib = N.load()
    for n in names:
        assert getattr(lib, n).restype is N.C.c_int
    assert callable(N.UpdateGroup) and all(hasattr(N.UpdateGroup, k) for k in ("run", "finish", "placement", "close"))
    from ddrl_amd.population import PopulationTrainer
    assert all(hasattr(PopulationTrainer, k) for k in ("train", "save", "restore", "stop"))
