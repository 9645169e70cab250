"""Byte text with degenerate and arbitrary 256-entry tables (tests/hasher_cases.py: const, two, low16, random at rot 0,
16, 17 and 31, non-zero xor terms) against the definition-level numpy checker (tests/text_checker.py): single texts
around the text tile of 8 192 windows, fused and generic, all modes, both strands, super-k-mer indices; one record
batch; and the constant table's one output per window."""
import numpy as np
import pytest

import hasher_cases as hc
import text_checker as tc

pytestmark = pytest.mark.gpu

SENT = -7
TILE = 8192  # windows of a text tile
PLANS = [(21, 11), (5, 5), (31, 19)]


@pytest.fixture(scope="module", autouse=True)
def _nothing_compiled(sm, gpu):
    before = sm.jit_stats()
    for canonical in (False, True):
        assert {w for _, w in PLANS} <= set(sm.text_prebuilt_window_sizes(canonical))
    yield
    after = sm.jit_stats()
    assert (after["compiled"], after["failed"]) == (before["compiled"], before["failed"]), (before, after)


def _filled(n):
    import torch
    return torch.full((n,), SENT, dtype=torch.int32, device="cuda")


def _same(out, count, want, tag):
    assert count == len(want), (tag, count, len(want))
    host = out[: count + 1].cpu().numpy()
    assert np.array_equal(host[:count].view(np.uint32), want), tag
    assert host[count] == SENT, tag


def _case(i, canonical):
    """case i of the text rotation, always with non-zero xor terms"""
    c = hc.nth(i, canonical, seed=81, size=256, families=hc.TEXT_FAMILIES, rots=hc.TEXT_ROTS)
    return hc.Case(c.family, c.rot, canonical, c.seed, xor=True, size=256)


def test_text_tables_single_text(sm, gpu):
    import torch
    uniform = np.random.default_rng(8201).integers(0, 256, 2 * TILE + 200, dtype=np.uint8)
    english = tc.english_like(2 * TILE + 200, 8202)
    d_text = {"uniform": torch.from_numpy(uniform).cuda(), "english": torch.from_numpy(english).cuda()}
    h_text = {"uniform": uniform, "english": english}
    fused, generic = (hc.Tally(hc.TEXT_FAMILIES, hc.TEXT_ROTS) for _ in range(2))
    i = redo = sks = 0
    for k, w in PLANS:
        l = k + w - 1
        lengths = [TILE * t + d + l - 1 for t in (1, 2) for d in (-1, 0, 1)] + [l - 1]
        for mode in (0, 1, 2):
            for canonical in (False, True):
                for n in lengths:
                    case = _case(i, canonical)
                    which = ("uniform", "english")[i & 1]
                    i += 1
                    th = case.product(sm)
                    sk = mode == 0
                    want = tc.run(h_text[which][:n], k, w, th, canonical, mode, super_kmers=sk)
                    b = sm.Builder(k, w, canonical, mode, text_hasher=th)
                    nw = max(0, n - l + 1)
                    for forced in (False, True):
                        tag = (case, which, k, w, mode, canonical, n, forced)
                        out = _filled(nw + 8)
                        osk = _filled(nw + 8) if sk else None
                        gpu.force_generic(forced)
                        try:
                            c = b.run_text_device(d_text[which], n, out, out_sk=osk)
                            if nw:
                                assert gpu.last_path() == (sm.PATH_GENERIC if forced else sm.PATH_FUSED), tag
                        finally:
                            gpu.force_generic(False)
                        if sk:
                            _same(out, c, want[0], tag)
                            _same(osk, c, want[1], tag)
                            sks += 1
                        else:
                            _same(out, c, want, tag)
                        if nw:
                            (generic if forced else fused).add(case, n, c)
        # every key ties, forward windows select the leftmost k-mer: one output per window
        for t, rot in ((2, 0), (1, 16), (2, 17), (1, 31)):
            n = TILE * t + 1 + l - 1
            case = hc.Case("const", rot, False, seed=90 + k, xor=True, size=256)
            b = sm.Builder(k, w, False, 0, text_hasher=case.product(sm))
            out = _filled(n - l + 1 + 8)
            c = b.run_text_device(d_text["uniform"], n, out)
            assert gpu.last_path() == sm.PATH_FUSED
            assert c == n - l + 1, (case, k, w, n)
            _same(out, c, np.arange(n - l + 1, dtype=np.uint32), (case, k, w, n))
            fused.add(case, n, c)
            redo += 1
    print("super-k-mer checks", sks, "one-output-per-window runs", redo)
    fused.check("text, fused")
    generic.check("text, generic")
    assert redo == 12 and sks >= 80


def test_text_tables_record_batch(sm, gpu):
    """One batch of the record lengths of tests/test_gpu_text_batch.py under the const and the random tables."""
    import torch
    k, w = 21, 11
    l = k + w - 1
    rng = np.random.default_rng(8203)
    lens = [0, 1, l - 1, l, l + 1, 8191, 8192, 8193, 20_000, 2 * l, 3, 100, 5000]
    lens = [int(x) for x in rng.permutation(lens)]
    lens[3:3] = [0] * 7
    lens += [0] * 5 + [l + 2]
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(starts[-1])
    text = rng.integers(0, 256, n, dtype=np.uint8)
    d_text, d_starts = torch.from_numpy(text).cuda(), torch.from_numpy(starts).cuda()
    tally = hc.Tally(("const", "random"), (0, 16, 17, 31))
    for i, (family, rot) in enumerate([("const", 0), ("random", 16), ("const", 17), ("random", 31), ("const", 16),
                                       ("random", 0)]):
        canonical = bool(i & 1)
        mode = (0, 0, 1, 2, 0, 0)[i]
        sk = mode == 0
        case = hc.Case(family, rot, canonical, seed=95 + i, xor=True, size=256)
        th = case.product(sm)
        b = sm.Builder(k, w, canonical, mode, text_hasher=th)
        out, osk = _filled(n + 8), (_filled(n + 8) if sk else None)
        offs = torch.full((len(lens) + 1,), -1, dtype=torch.int64, device="cuda")
        cnt = sm.run_text_batch_device(b, d_text, d_starts, n, out, offs, out_sk=osk)
        assert gpu.last_path() == sm.PATH_FUSED
        ho = offs.cpu().numpy()
        hp = out[: cnt + 1].cpu().numpy()
        assert ho[0] == 0 and ho[-1] == cnt and hp[cnt] == SENT
        hs = osk[: cnt + 1].cpu().numpy() if sk else None
        for r, m in enumerate(lens):
            want = tc.run(text[starts[r]: starts[r] + m], k, w, th, canonical, mode, super_kmers=sk)
            got = hp[ho[r]:ho[r + 1]].view(np.uint32)
            if sk:
                assert np.array_equal(got, want[0]), (case, r, m)
                assert np.array_equal(hs[ho[r]:ho[r + 1]].view(np.uint32), want[1]), (case, r, m)
            else:
                assert np.array_equal(got, want), (case, r, m)
            if family == "const" and mode == 0 and not canonical:
                assert len(got) == max(0, m - l + 1), (case, r, m)
        if sk:
            assert hs[cnt] == SENT
        tally.add(case, n, cnt)
    tally.check("text, record batch")
