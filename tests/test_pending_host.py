"""CPU tests of irec.coding.pending: PendingCodes built by hand on host tensors through the five gathers (`gather` and the four
`gather_packed*`), and `recode` over fake passes.  Every expectation is stated here in plain Python / numpy from the rule itself:
which error a pass raises (a MorePartitionsNeeded wins over a SplitNotResident, the largest need among several), which coders step
back (every distinct one once, when any call gave up), what every coder's hints are afterwards (every call's check runs), and where
a row lands (image-major, call, natural block order, zero-padded to the widest call)."""
import itertools

import numpy as np
import pytest
import torch

import rec_ragged_cases as C

pytestmark = [pytest.mark.both_suites, pytest.mark.usefixtures("suite")]

LAYOUTS = {"even": ("cpu", 2, 8, 4, 42), "short_tail": ("cpu", 2, 10, 4, 42)}       # blocks of 4, 4 | 4, 4, 2 dims: 2 tensors each
GATHERS = ["gather", "gather_packed", "gather_packed_device", "gather_packed_ragged", "gather_packed_ragged_device"]
KINDS = {"whole": (2, 2), "gave_up": (-2, 2), "needs3": (3, 2), "needs5": (5, 4)}   # (the K of the call's marked row, its max_K)
PASSES = [p for n in (2, 3) for p in itertools.permutations(KINDS, n)]


class Coder(C.StubCoder):
    """StubCoder with what a pass that gave up asks of its coders."""

    def __init__(self):
        super().__init__()
        self.stepped_back = 0

    def _split_gave_up(self):
        self.stepped_back += 1

    def _engine_for(self, tensor):
        raise AssertionError("an unshared call with extrapolated ratios asks for no engine")


def _layout(name):
    from irec.engine import BlockLayout
    return BlockLayout(*LAYOUTS[name])


def _call(coder, lay, width, tag, r=0, marked=None):
    """A call whose row of natural block (i, j) says so itself: K = (i + j + r) % (width + 1), idx[t] = tag + 100 i + 10 j + t; `marked`
    replaces the K of natural block (1, 1)."""
    from irec.coding.beam_search_coder import PendingCode
    bpt = lay.blocks_per_tensor
    K = torch.zeros(lay.n_blocks, dtype=torch.int32)
    idx = torch.full((lay.n_blocks, width), -7, dtype=torch.int32)
    for i in range(lay.n_tensors):
        for j in range(bpt):
            row = int(lay.natural[i * bpt + j])
            K[row] = (i + j + r) % (width + 1)
            idx[row] = torch.arange(width, dtype=torch.int32) + tag + 100 * i + 10 * j
    if marked is not None:
        K[int(lay.natural[bpt + 1])] = marked
    return PendingCode(coder, lay, K, idx, None, width)


def _want_K(lay, width, r, marked=None):
    K = np.array([[(i + j + r) % (width + 1) for j in range(lay.blocks_per_tensor)] for i in range(lay.n_tensors)], dtype=np.int32)
    if marked is not None:
        K[1, 1] = marked
    return K


# ---- precedence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_coders", [1, 2], ids=["one_coder", "two_coders"])
@pytest.mark.parametrize("kinds", PASSES, ids="-".join)
@pytest.mark.parametrize("gather", GATHERS)
def test_one_precedence_rule_in_every_gather(gather, kinds, n_coders):
    """Passes of two or three calls of different kinds, in every order, on one coder or two in turn.  (`gather` once kept a copy of
    this rule of its own, which read `.need` off a SplitNotResident when a give-up came before a needs-more.)"""
    from irec.coding.beam_search_coder import MorePartitionsNeeded, PendingCode, SplitNotResident
    lay = _layout("short_tail")
    coders = [Coder() for _ in range(n_coders)]
    pend = [_call(coders[r % n_coders], lay, KINDS[k][1], 1000 * r, r, marked=KINDS[k][0]) for r, k in enumerate(kinds)]
    needs = [KINDS[k][0] for k in kinds if k.startswith("needs")]
    gave_up = "gave_up" in kinds
    fn = getattr(PendingCode, gather)
    if needs:
        with pytest.raises(MorePartitionsNeeded) as e:
            fn(pend)
        assert e.value.need == max(needs)
    elif gave_up:
        with pytest.raises(SplitNotResident):
            fn(pend)
    else:
        fn(pend)
    for c, coder in enumerate(coders):
        mine = [(r, k) for r, k in enumerate(kinds) if r % n_coders == c and k != "gave_up"]      # a call that gave up touches no hint
        assert coder.stepped_back == (1 if gave_up else 0)
        assert coder._K_reads == len(mine)
        assert coder._max_K_hint == max([int(_want_K(lay, KINDS[k][1], r, KINDS[k][0]).max()) for r, k in mine], default=0)


# ---- results -----------------------------------------------------------------------------------------------------------------------
def _whole_pass(names, min_indices=0):
    """Three whole calls of widths 2, 3, 4 on the layouts `names` (one name: all on it); returns (pendings, want K [N, T], want idx
    [N, T, 4] zero-padded, blocks_per_res, widths) with T the calls' blocks side by side -- the row order said in numpy."""
    lays = {n: _layout(n) for n in set(names)}
    coder, widths = Coder(), (2, 3, 4)
    pend = [_call(coder, lays[n], w, 1000 * (r + 1), r) for r, (n, w) in enumerate(zip(names, widths))]
    for p in pend:
        p.min_indices = min_indices
    bpr = [p.lay.blocks_per_tensor for p in pend]
    K = np.concatenate([_want_K(p.lay, w, r) for r, (p, w) in enumerate(zip(pend, widths))], axis=1)
    idx = np.zeros((2, sum(bpr), 4), dtype=np.int32)
    at = 0
    for r, (b, w) in enumerate(zip(bpr, widths)):
        for i in range(2):
            for j in range(b):
                idx[i, at + j, :w] = 1000 * (r + 1) + 100 * i + 10 * j + np.arange(w)
        at += b
    assert K.min() == 0 and K.max() == 4                      # rows without an index and a full widest row are both there
    return pend, np.maximum(K, min_indices), idx, bpr, widths


def _is_joined_view(K, idx):
    return K.data_ptr() + 4 == idx.data_ptr() and K.stride(-1) == 5 and idx.stride()[-2:] == (5, 1)


@pytest.mark.parametrize("min_indices", [0, 1])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_uniform_gathers_against_the_row_order_in_numpy(name, min_indices):
    from irec.coding.beam_search_coder import PendingCode
    pend, K, idx, bpr, widths = _whole_pass([name] * 3, min_indices)
    bpt = bpr[0]
    K, idx = K.reshape(2, 3, bpt), idx.reshape(2, 3, bpt, 4)
    lists = PendingCode.gather(pend)                                                       # [call][image][block]
    assert lists == [[[idx[i, r, j, :K[i, r, j]].tolist() for j in range(bpt)] for i in range(2)] for r in range(3)]
    assert all(len(ix) <= widths[r] for r in range(3) for img in lists[r] for ix in img)
    Kh, ih = PendingCode.gather_packed(pend)
    assert Kh.dtype == np.int32 and ih.dtype == np.int32 and Kh.flags.c_contiguous and ih.flags.c_contiguous
    assert np.array_equal(Kh, K) and np.array_equal(ih, idx)                               # (idx: the narrower calls zero-padded)
    Kd, idd = PendingCode.gather_packed_device(pend)
    assert np.array_equal(Kd.numpy(), K) and np.array_equal(idd.numpy(), idx) and _is_joined_view(Kd, idd)
    assert pend[0].coder._max_K_hint == 4 and pend[0].coder._K_reads == 9                  # three gathers of three calls
    assert int(pend[0].K.min()) == 0                                                       # the clamp is on the gathered rows alone


@pytest.mark.parametrize("min_indices", [0, 1])
@pytest.mark.parametrize("names", [("even", "short_tail", "even"), ("short_tail", "even", "short_tail")], ids="-".join)
def test_ragged_gathers_against_the_row_order_in_numpy(names, min_indices):
    from irec.coding.beam_search_coder import PendingCode
    pend, K, idx, bpr, _ = _whole_pass(names, min_indices)
    Kh, ih, bpr_h = PendingCode.gather_packed_ragged(pend)
    assert bpr_h == bpr and Kh.dtype == np.int32 and ih.dtype == np.int32 and Kh.flags.c_contiguous and ih.flags.c_contiguous
    assert np.array_equal(Kh, K) and np.array_equal(ih, idx)
    Kd, idd, bpr_d = PendingCode.gather_packed_ragged_device(pend)
    assert bpr_d == bpr and np.array_equal(Kd.numpy(), K) and np.array_equal(idd.numpy(), idx) and _is_joined_view(Kd, idd)
    lists = PendingCode.gather(pend)                                                       # the list form of the same pass
    first = np.concatenate([[0], np.cumsum(bpr)])
    assert lists == [[[idx[i, first[r] + j, :K[i, first[r] + j]].tolist() for j in range(bpr[r])] for i in range(2)] for r in range(3)]
    assert len(pend[0].lay.__dict__["_ragged_index"]) == 1                                 # the row index is built once per pass shape


# ---- recode --------------------------------------------------------------------------------------------------------------------------
def _fake_pass(failures):
    """(code_pass, gather, calls): a pass whose read-back raises failures[i] at its i-th try and is whole afterwards."""
    calls = []

    def code_pass():
        calls.append(len(calls))
        return ["pending", len(calls)], ("rest", len(calls))

    def gather(pendings):
        assert pendings == ["pending", len(calls)]
        if len(calls) <= len(failures):
            raise failures[len(calls) - 1]
        return ("gathered", len(calls))

    return code_pass, gather, calls


@pytest.mark.parametrize("k", range(6))
def test_recode_returns_after_k_failures(k):
    from irec.coding.beam_search_coder import MorePartitionsNeeded, SplitNotResident
    from irec.coding.pending import recode
    failures = [MorePartitionsNeeded(40 + i) if i % 2 else SplitNotResident("partners not resident") for i in range(k)]
    code_pass, gather, calls = _fake_pass(failures)
    assert recode(code_pass, gather, [Coder()]) == (("gathered", k + 1), ("rest", k + 1)) and len(calls) == k + 1


def test_recode_gives_up_after_six_failures():
    from irec.coding.beam_search_coder import MorePartitionsNeeded, SplitNotResident
    from irec.coding.pending import recode
    coders = [Coder(), Coder(), Coder()]
    for c, hint in zip(coders, (7, 41, 12)):
        c._max_K_hint = hint
    for failures in ([MorePartitionsNeeded(50)] * 6, [SplitNotResident("partners not resident")] * 6):
        code_pass, gather, calls = _fake_pass(failures)
        with pytest.raises(MorePartitionsNeeded) as e:
            recode(code_pass, gather, coders)
        assert e.value.need == 42 and len(calls) == 6
    code_pass, gather, calls = _fake_pass([MorePartitionsNeeded(50)] * 3)                   # attempts is the caller's to lower
    with pytest.raises(MorePartitionsNeeded) as e:
        recode(code_pass, gather, coders, attempts=3)
    assert e.value.need == 42 and len(calls) == 3


@pytest.mark.parametrize("error", ["CodingError", "ValueError", "AttributeError"])
def test_recode_catches_nothing_else(error):
    from irec.coding.pending import recode
    from irec.coding.utils import CodingError
    kind = {"CodingError": CodingError, "ValueError": ValueError, "AttributeError": AttributeError}[error]
    code_pass, gather, calls = _fake_pass([kind("not a recode")])
    with pytest.raises(kind, match="not a recode") as e:
        recode(code_pass, gather, [Coder()])
    assert type(e.value) is kind and len(calls) == 1
