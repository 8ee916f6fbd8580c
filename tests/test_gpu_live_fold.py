"""K4m csr_merge (csrc/index_merge.hip): the live index's delta folded into main without a sort. The folded CSR must
equal, bit for bit, the numpy stable-sort mirror of the stored postings (as test_gpu_match.py
test_csr_layout_equals_stable_mirror) and the CSR a second engine builds once from the same postings. Constructed
postings place buckets at the edges of the merge's work split: 1024 keys per tile and 8192 destination postings per
work item (aidfp_live_plan.h kMergeTileKeys, kMergeItemPosts)."""

import numpy as np
import pytest

import k5_fixtures as F
import oracle as O
from aidfp.engine import Engine
from store_ref import csr_mirror

pytestmark = pytest.mark.gpu
SR = 16000
TILE, ITEM = 1024, 8192
KEYS = 1 << 26


def hash_of_key(key):
    """The inverse of aidfp_layout.h bucket_key (a bit permutation of the 26 bits a hash can set)."""
    k = np.asarray(key, dtype=np.int64)
    h = (((k >> 18) & 0xFF) << 22) | (((k >> 16) & 3) << 30) | (((k >> 9) & 0x7F) << 12) | (((k >> 6) & 7) << 19) | (k & 0x3F)
    assert np.array_equal(F.bucket_key(h), k)
    return h.astype(np.uint32)


def postings(runs, track0, seed):
    """runs: (key, count) pairs -> [n, 3] postings in a shuffled arrival order; t numbers the postings, so every one
    is distinct and a bucket's arrival order shows in the CSR; tracks track0 .. track0 + 6."""
    keys = np.repeat([k for k, _ in runs], [c for _, c in runs]).astype(np.int64)
    rng = np.random.default_rng(seed)
    keys = keys[rng.permutation(len(keys))]
    n = len(keys)
    return np.stack([hash_of_key(keys), (track0 + np.arange(n) % 7).astype(np.uint32), np.arange(n, dtype=np.uint32)],
                    axis=1).astype(np.uint32)


def add(eng, post):
    if len(post):
        h, tr, t = F.columns(post)
        eng.index_add_postings(h.ctypes.data, tr.ctypes.data, t.ctypes.data, len(post), device=False)


def check_csr(eng, post, removed=()):
    offs, posts = eng.index_csr()
    ref_offs, ref_posts = csr_mirror(post, removed)
    assert len(posts) == len(ref_posts)
    bad = np.flatnonzero(posts != ref_posts)
    assert len(bad) == 0, f"{len(bad)} CSR postings out of place, first at {bad[:5]}"
    assert np.array_equal(offs, ref_offs)
    return offs, posts


T20 = 20 * TILE  # a tile of its own for the item-boundary cases
MAIN_RUNS = [(0, 3), (KEYS - 1, 1),            # the first and the last key
             (TILE - 1, 5), (2 * TILE - 1, 2),  # both sides of a tile boundary: main only, then both
             (5000, ITEM + 1),                  # a bucket one posting longer than a work item, in main
             (T20, ITEM),                       # an item boundary exactly at a bucket's end (the tile's first bucket)
             (T20 + 1, 50), (T20 + 10, 5000),   # ... and the next one inside bucket T20 + 10 (8342 .. 18342 of the tile)
             (40000, 1), (40001, 1), (40003, 2)]
DELTA_RUNS = [(0, 2), (KEYS - 1, 4),
              (TILE, 6), (2 * TILE - 1, 3),     # delta only, then both
              (9000, ITEM + 1),                 # one posting longer than a work item, in the delta
              (T20 + 1, 100), (T20 + 10, 5000),
              (40001, 3), (40002, 1)]          # neighbours: main only, both, delta only, main only


def test_fold_equals_the_full_build():
    main, delta = postings(MAIN_RUNS, 0, 1), postings(DELTA_RUNS, 100, 2)
    with Engine(SR, min_match=1) as live, Engine(SR, min_match=1) as one:
        add(live, main)
        live.index_finalize()
        live.index_live(1 << 22)
        add(live, delta)
        rec = F.records(hash_of_key([2 * TILE - 1, T20 + 1, KEYS - 1]), [0, 0, 0])
        two_pass = live.query([rec])[0]  # over main + delta
        live.index_finalize()            # the fold
        st = live.index_live_stats()
        assert (st["main_builds"], st["delta_builds"], st["folds"]) == (1, 1, 1), st
        assert (st["main_postings"], st["delta_postings"]) == (len(main) + len(delta), 0), st
        offs, posts = check_csr(live, np.concatenate([main, delta]))
        add(one, main)
        add(one, delta)
        one.index_finalize()
        o1, p1 = one.index_csr()
        assert np.array_equal(posts, p1) and np.array_equal(offs, o1)
        # the signatures were carried with their postings: the LDS path reads them
        got = live.query([rec])[0]
        want = O.query(one.index_export(), rec, min_match=1, max_rows=one.max_results)
        assert len(want) == 14 and np.array_equal(got, want) and np.array_equal(two_pass, want)
        assert live.match_stats()["queries_global"] == 0


def test_fold_with_an_empty_delta_and_a_second_fold():
    """The cap-triggered fold (a query runs it). A delta whose only track was removed is empty when the fold builds it:
    the merge copies main. The next fold writes into the buffers the first one replaced."""
    main = postings([(7, 4), (TILE + 3, 9), (70000, 2)], 0, 3)
    gone = postings([(7, 30), (90000, 30)], 100, 4)  # 60 postings, tracks 100 .. 106
    more = postings([(7, 3), (TILE + 3, 1), (TILE + 4, 25), (KEYS - 2, 12)], 200, 5)
    rec = F.records(hash_of_key([7]), [0])
    with Engine(SR, min_match=1) as live:
        add(live, main)
        live.index_finalize()
        live.index_live(40)
        add(live, gone)
        for t in range(100, 107):
            live.index_remove(t)
        rows = live.query([rec])[0]  # tail 60 > 40: the fold, over an empty delta
        st = live.index_live_stats()
        assert (st["main_builds"], st["delta_builds"], st["folds"], st["delta_postings"]) == (1, 1, 1, 0), st
        assert sorted(rows[:, 1].tolist()) == sorted(set(main[F.bucket_key(main[:, 0]) == 7][:, 1].tolist()))
        assert live.index_stats()["live"] == len(main)
        check_csr(live, live.index_export(), removed=range(100, 107))
        add(live, more)  # tail 41 > 40
        live.query([rec])
        st = live.index_live_stats()
        assert (st["main_builds"], st["delta_builds"], st["folds"], st["delta_postings"]) == (1, 2, 2, 0), st
        check_csr(live, live.index_export(), removed=range(100, 107))
        assert np.array_equal(live.query([rec])[0],
                              O.query(np.concatenate([main, more]), rec, min_match=1, max_rows=live.max_results))


def test_fold_into_a_main_of_zero_postings():
    delta = postings([(0, 1), (3, 2), (TILE, 1), (KEYS - 1, 2), (123456, ITEM + 3)], 0, 6)
    with Engine(SR) as live:
        live.index_finalize()  # main over nothing
        live.index_live(1 << 20)
        add(live, delta)
        live.index_finalize()
        st = live.index_live_stats()
        assert (st["main_builds"], st["delta_builds"], st["folds"], st["main_postings"]) == (1, 1, 1, len(delta)), st
        check_csr(live, delta)
