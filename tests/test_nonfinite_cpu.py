"""The premises of tests/test_nonfinite_gpu.py, without a GPU: every case tests both rules of tests/nonfinite_cases.py (its
float64 reference has a non-finite element to launder and an output that is at least half finite to damage, or the case says
that the operation absorbs that poison), the non-finite mask of a case does not depend on the precision the reference runs in
(inputs are of standard-normal scale: nothing overflows except through the poison) -- but for the padding taps of the
convolutions, which torch's float32 kernels skip and its float64 kernels multiply by zero and which neither rule looks at
(nonfinite_cases.Case.reference) -- and ``compare`` itself fails on a laundered and on a collateral result."""
import collections

import pytest
import torch

from tests import nonfinite_cases as N

GROUPS = N.groups()


def test_poison_replaces_one_element_of_a_copy():
    t = torch.arange(24.0).view(2, 3, 4)
    for kind, value in N.VALUES.items():
        for where, index in (("first", 0), ("last", 23), ("interior", 10)):
            p = N.poison(t, kind, where)
            assert p.shape == t.shape and p.data_ptr() != t.data_ptr() and bool(torch.isfinite(t).all())
            bad = N.nonfinite(p).view(-1).nonzero().view(-1).tolist()
            assert bad == [index]
            assert (p.view(-1)[index] != p.view(-1)[index]) if kind == "nan" else float(p.view(-1)[index]) == value
            keep = torch.ones(24, dtype=torch.bool)
            keep[index] = False
            assert torch.equal(p.view(-1)[keep], t.view(-1)[keep])


def _premises(case, target, kind, where):
    """-> True when the reference absorbs the poison (every output finite)"""
    what = "%s %s %s@%s" % (case.name, target, kind, where)
    inp = case.poisoned(target, kind, where)
    assert int(N.nonfinite(inp[target]).sum()) == 1 and all(bool(torch.isfinite(v).all()) for k, v in inp.items() if k != target), what
    ref64, exempt = case.reference(inp, target)
    ref32 = case.torch(inp, torch.float32)
    assert set(exempt) <= set(ref64) and list(ref64) == list(ref32), what
    some_bad, half_finite = False, False
    for name, r in ref64.items():
        m64, m32 = N.nonfinite(r), N.nonfinite(ref32[name])
        skip = exempt.get(name, torch.zeros_like(m64))
        # outside the exempt elements (products of the poison with a zero from beyond the other operand's range, which torch's
        # float32 and float64 kernels treat differently: Case.reference) the mask is the same in both precisions
        assert torch.equal(m64 & ~skip, m32 & ~skip), "%s %s: the non-finite mask depends on the precision (%d float64, %d float32)" % (
            what, name, int((m64 & ~skip).sum()), int((m32 & ~skip).sum()))
        some_bad |= bool((m64 & ~skip).any())
        half_finite |= 2 * int((~m64 & ~skip).sum()) >= m64.numel()
    assert half_finite, what + ": no output is half finite, rule 2 would test nothing"
    return not some_bad


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_case_tests_both_rules_and_its_mask_is_precision_independent(group):
    for case in GROUPS[group]():
        clean = case.torch(case.inputs, torch.float64)
        assert all(bool(torch.isfinite(v).all()) for v in clean.values() if v is not None), case.name
        for target in case.targets:
            absorbed = {(kind, where): _premises(case, target, kind, where) for kind, where in N.POISONS}
            for (kind, where), a in absorbed.items():
                assert a == ((target, kind) in case.absorbs), "%s %s %s@%s: absorbed %s" % (case.name, target, kind, where, a)
            assert not all(absorbed.values()), "%s %s: no poison reaches an output, rule 1 would test nothing" % (case.name, target)


@pytest.mark.parametrize("geo", list(N.POOL_POSITIONS), ids=lambda g: "k%ds%dp%d" % g)
def test_pool_cases(geo):
    x, g = N.pool_inputs()
    go = torch.randint(-4, 5, (N.POOL_SHAPE[0], N.POOL_SHAPE[1]) + N.pool_out_size(geo), generator=g).float()
    for kind, value in N.VALUES.items():
        for (py, px) in N.POOL_POSITIONS[geo]:
            xp = x.clone()
            xp[0, 1, py, px] = value
            r64, r32 = N.pool_reference(xp, go, geo), N.pool_reference(xp, go, geo, torch.float32)
            for name in r64:
                assert torch.equal(N.nonfinite(r64[name]), N.nonfinite(r32[name]))   # and, selection being exact, the same values
                assert torch.equal(torch.nan_to_num(r64[name].float(), 7.0, 8.0, 9.0), torch.nan_to_num(r32[name], 7.0, 8.0, 9.0))
            covered = not (geo == (2, 2, 0) and (py, px) == (4, 6))
            if kind != "-inf":
                assert bool(N.nonfinite(r64["y"]).any()) == covered, (kind, py, px)
            assert bool(torch.isfinite(r64["grad_x"]).all())   # the gradient selects: no product with the poison
        gp = go.clone()
        gp.view(-1)[3] = value
        r = N.pool_reference(x, gp, geo)
        assert int(N.nonfinite(r["grad_x"]).sum()) == 1 and bool(torch.isfinite(r["y"]).all())


def test_compare_fails_on_a_laundered_and_on_a_collateral_result():
    g = torch.Generator().manual_seed(1)
    ref = collections.OrderedDict(a=torch.randn(4, 5, generator=g).double(), b=torch.randn(7, generator=g).double())
    ref["a"][1, 2] = float("nan")
    ref["a"][3, 0] = float("inf")
    good = collections.OrderedDict((k, v.float()) for k, v in ref.items())
    stats = N.compare(good, ref, 1e-4, "good")
    assert stats["a"].ref_nonfinite == 2 and stats["a"].laundered == 0 and stats["a"].missed == 0 and stats["b"].worst <= 1e-2
    swapped = collections.OrderedDict((k, v.clone()) for k, v in good.items())   # Inf against NaN is no difference
    swapped["a"][1, 2], swapped["a"][3, 0] = float("-inf"), float("nan")
    N.compare(swapped, ref, 1e-4, "class swapped")
    laundered = collections.OrderedDict((k, v.clone()) for k, v in good.items())
    laundered["a"][1, 2] = 0.0
    with pytest.raises(AssertionError, match="rule 1"):
        N.compare(laundered, ref, 1e-4, "laundered")
    collateral = collections.OrderedDict((k, v.clone()) for k, v in good.items())
    collateral["b"][4] += 1e-3 * float(ref["b"].abs().max())
    with pytest.raises(AssertionError, match="rule 2"):
        N.compare(collateral, ref, 1e-4, "collateral")
    assert N.compare(collateral, ref, 1e-4, "collateral, counted only", collateral=False)["b"].missed == 1
    spread = collections.OrderedDict((k, v.clone()) for k, v in good.items())    # a finite reference element made non-finite
    spread["b"][0] = float("nan")
    with pytest.raises(AssertionError, match="rule 2"):
        N.compare(spread, ref, 1e-4, "spread")
    exact = collections.OrderedDict(a=ref["a"].float().double())
    N.compare(collections.OrderedDict(a=ref["a"].float()), exact, 0.0, "exact")
    off = ref["a"].float()
    off[0, 0] += 1e-6
    with pytest.raises(AssertionError, match="rule 2"):
        N.compare(collections.OrderedDict(a=off), exact, 0.0, "exact, one ulp off")
