"""One-pass window sums (csrc/segsum.hip wsum_onepass_kernel) against the device two-kernel
path (chunk_totals + chunk_windows) on the same inputs: every comparison is bitwise."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LV = np.array([0.0, 1.0])


def _mi(y, m):
    from pfml.utils.dates import mi_from_ym
    return mi_from_ym(y, m)


def _span(y0, m0, y1, m1):
    return np.arange(_mi(y0, m0), _mi(y1, m1) + 1, dtype=np.int64)


def _setup(months, years, G, dev, world=1, rank=0, rows=None):
    from pfml.models.search import _search_setup
    rows = np.arange(len(months)) if rows is None else rows
    return _search_setup(months, np.asarray(years), [16], G, len(rows), world, rank,
                         torch.device(dev), LV, rows)


def _inputs(G, T, P, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn(G, T, P, P, generator=g, dtype=torch.float64, device=dev)
    X = (X + X.transpose(-1, -2)).contiguous()
    R = torch.randn(G, T, P, generator=g, dtype=torch.float64, device=dev)
    return X, R


def _two_kernel(X, R, su):
    from pfml.ops.wsum import chunk_totals, chunk_windows
    totD, totR, bufs = chunk_totals(X, R, su.win)
    return chunk_windows(X, R, su.win, totD, totR, bufs)


def _check_bitwise(X, R, su):
    from pfml.ops.wsum import window_sums_onepass
    refD, refR = _two_kernel(X, R, su)
    SD, Sr = window_sums_onepass(X, R, su.win)
    assert SD.shape == refD.shape and Sr.shape == refR.shape
    assert torch.equal(Sr, refR)
    assert torch.equal(SD, refD)
    return SD, Sr


MONTHS1, YEARS1 = _span(1990, 0, 2012, 11), np.arange(1998, 2012)


@pytest.mark.parametrize("P", [1, 31, 32, 33, 65, 97])
def test_onepass_p_sweep(gpu, P):
    """P = 1 (a one-element tile), 31 / 33 / 65 / 97 (ragged last tiles; odd row and month
    pitches, so the 16-byte loads sit on 8-byte boundaries) and 32 (even pitch), G = 2, the
    months and hp years of test_chunked_window_sums_world_bitwise."""
    su = _setup(MONTHS1, YEARS1, 2, gpu)
    X, R = _inputs(2, len(MONTHS1), P, gpu, 100 + P)
    _check_bitwise(X, R, su)


def _gappy_months():
    drop = {_mi(1996, 2), _mi(1996, 5), _mi(1996, 6), _mi(1996, 10), _mi(1998, 7)}
    return np.array([t for t in range(_mi(1991, 0), _mi(2000, 5) + 1) if t not in drop],
                    dtype=np.int64)


# (months, hp years, burn-in piece lengths the layout must have)
BURN_CASES = {
    # year blocks of 12, 8, 12, 11, 12 months level the eight pieces at 13 months each
    "odd_pieces": (_gappy_months, np.arange(1996, 2001), [1, 5, 1, 2, 1, 13, 13, 12]),
    # 21 burn-in months: all of them go to the three chunks without a year
    "empty_pieces": (lambda: _span(1993, 3, 2000, 5), np.arange(1996, 2001),
                     [0, 0, 0, 0, 0, 7, 7, 7]),
}


@pytest.mark.parametrize("case", sorted(BURN_CASES))
def test_onepass_burn_in_lengths(gpu, case):
    """Burn-in pieces of 1, 2, 5, 13 (and 7, 12) months: leftovers after the groups of four,
    a piece shorter than one group, pieces longer than one trip of twelve; empty pieces; year
    chunks without a year (ys == ye).  One layout cannot have an empty piece, a 13-month piece
    and an empty year chunk together (an empty year chunk means at most seven hp years, so no
    chunk holds more than twelve block months, and the pieces level every chunk), hence two
    layouts; each is asserted to have the properties it is here for."""
    from pfml.models.search import make_plan, win_layout
    mk, years, want = BURN_CASES[case]
    months = mk()
    lay = win_layout(make_plan(months, years), len(years), 1)
    lens = [b - a for a, b in lay.burn]
    assert lens == want
    assert any(len(c) == 0 for c in lay.ychunks)
    if case == "odd_pieces":
        assert {1, 5, 13} <= set(lens) and all(n % 4 for n in lens if n != 12)
    else:
        assert 0 in lens and all(n % 4 for n in lens if n)
    su = _setup(months, years, 2, gpu)
    assert any(int(a) == int(b) for a, b in zip(su.win.ys, su.win.ye))
    X, R = _inputs(2, len(months), 45, gpu, 7)
    _check_bitwise(X, R, su)


def test_onepass_trailing_validation_months(gpu):
    """Months that end inside the validation year of the last hp year (the months after the
    last block feed no window): nine hp years, so nseg - skip and nYl are 9 against case 1's
    14 and the first year chunk holds two years.  (clast is C - 1 on every one-rank layout
    with at least one hp year: the rank owns all C chunks.)"""
    months, years = _span(1988, 2, 2004, 7), np.arange(1995, 2004)
    su = _setup(months, years, 2, gpu)
    s1 = _setup(MONTHS1, YEARS1, 2, gpu)
    assert su.nYl == 9 and su.win.nseg - su.win.skip == 9 and s1.nYl == 14
    assert int(max(su.win.sp)) < len(months)          # trailing months outside every segment
    assert su.win.clast == su.layout.C - 1
    X, R = _inputs(2, len(months), 37, gpu, 11)
    _check_bitwise(X, R, su)


@pytest.fixture(scope="module")
def case97(gpu):
    su = _setup(MONTHS1, YEARS1, 2, gpu)
    X, R = _inputs(2, len(MONTHS1), 97, gpu, 21)
    return su, X, R


def test_onepass_writes_every_element(gpu, case97, monkeypatch):
    """SD and Sr allocated full of NaN: the result has none and is symmetric, so every element
    is stored, the mirrored half and the ragged last tile (P = 97 = 64 + 33) included."""
    from pfml.ops import wsum
    su, X, R = case97
    real_empty = torch.empty

    def nan_empty(*a, **k):
        t = real_empty(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    monkeypatch.setattr(wsum.torch, "empty", nan_empty)
    SD, Sr = wsum.window_sums_onepass(X, R, su.win)
    monkeypatch.undo()
    assert not torch.isnan(SD).any() and not torch.isnan(Sr).any()
    assert torch.equal(SD, SD.transpose(-1, -2))
    refD, refR = _two_kernel(X, R, su)
    assert torch.equal(SD, refD) and torch.equal(Sr, refR)


def test_onepass_never_reads_lower_triangle(gpu, case97):
    """The strict lower triangle of every month set to NaN: bitwise the symmetric input's
    result."""
    from pfml.ops.wsum import window_sums_onepass
    su, X, R = case97
    P = X.shape[-1]
    low = torch.ones(P, P, dtype=torch.bool, device=gpu).tril(-1)
    Xn = X.masked_fill(low, float("nan"))
    SD, Sr = window_sums_onepass(X, R, su.win)
    SDn, Srn = window_sums_onepass(Xn, R, su.win)
    assert torch.equal(SDn, SD) and torch.equal(Srn, Sr)


def test_onepass_production_width(gpu):
    """P = 513 at small depth (G = 2, 40 months, 2 hp years): the ninth tile column (one
    column wide), the last tile row (one row high) and the workload's odd row pitch."""
    months, years = _span(1996, 0, 1999, 3), np.arange(1998, 2000)
    assert len(months) == 40
    su = _setup(months, years, 2, gpu)
    X, R = _inputs(2, len(months), 513, gpu, 31)
    SD, _ = _check_bitwise(X, R, su)
    assert torch.equal(SD, SD.transpose(-1, -2))


def _spy(monkeypatch, names):
    """Wrap the library handle's entry points; returns the list of the names called."""
    from pfml.ops import _native as nat
    lib = nat.hip_lib()
    seen = []

    def wrap(name):
        fn = getattr(lib, name)

        def call(*a):
            seen.append(name)
            return fn(*a)
        return call

    for n in names:
        monkeypatch.setattr(lib, n, wrap(n), raising=False)
    return seen


ENTRY = ["pfml_wsum_onepass", "pfml_wsum_chunk_totals", "pfml_wsum_chunk_prefix",
         "pfml_wvec_chunk"]


def test_onepass_switch(gpu, monkeypatch):
    """search.window_sums: the default takes pfml_wsum_onepass, PFML_WSUM_ONEPASS=0 the
    two-kernel entry points (bitwise the same windows), and a rank of a W = 2 run without a
    process group (the one-process rehearsal) the two-kernel path whatever the switch."""
    from pfml.models import search
    months, years = _span(1996, 0, 2001, 11), np.arange(1998, 2001)
    X, R = _inputs(2, len(months), 33, gpu, 41)
    su = _setup(months, years, 2, gpu)
    reals = search.PfmlReals(months=months, r_tilde=R, denom=X)
    assert search.dist_env().world_size == 1
    seen = _spy(monkeypatch, ENTRY)
    monkeypatch.delenv("PFML_WSUM_ONEPASS", raising=False)
    SD1, Sr1 = search.window_sums(reals, su.win)
    assert seen == ["pfml_wsum_onepass"]
    del seen[:]
    monkeypatch.setenv("PFML_WSUM_ONEPASS", "0")
    SD0, Sr0 = search.window_sums(reals, su.win)
    assert "pfml_wsum_onepass" not in seen
    assert {"pfml_wsum_chunk_totals", "pfml_wsum_chunk_prefix"} <= set(seen)
    assert torch.equal(SD1, SD0) and torch.equal(Sr1, Sr0)
    # rank 0 of a two-rank run, no process group
    del seen[:]
    monkeypatch.delenv("PFML_WSUM_ONEPASS", raising=False)
    rows = search.local_month_rows(months, years, 2, 0)
    su2 = _setup(months, years, 2, gpu, world=2, rank=0, rows=rows)
    reals2 = search.PfmlReals(months=months[rows], r_tilde=R[:, rows].contiguous(),
                              denom=X[:, rows].contiguous(), all_months=months)
    monkeypatch.setattr(search, "dist_env",
                        lambda: types.SimpleNamespace(world_size=2, rank=0, is_dist=False))
    search.window_sums(reals2, su2.win)
    assert "pfml_wsum_onepass" not in seen
    assert {"pfml_wsum_chunk_totals", "pfml_wsum_chunk_prefix"} <= set(seen)
