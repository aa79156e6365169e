"""The launch schedule a KktDevice builds before it uploads anything
(csrc/kkt_schedule.cpp, through ipo_hip_kkt_schedule; host code, no GPU).

The sync-free sweeps are persistent launches whose workgroups draw the items
of one list in order from a ticket counter, so they drain only if every item
waits solely on items earlier in its list.  The waits, restated from the
kernels (kkt_device.hip):
  k_fwd_sf, item of supernode s (whole, code -1, or one 64-row chunk, code =
      its solve chunk): waits until cnt[s] == epoch * need[s]; every forward
      item of a child c adds one to cnt[par[c]] when it ends.  So need[s] must
      count exactly the forward items of s's children inside the range, and
      all of them must come before every item of s.
  k_bwd_sf, item of s: waits until flag[par[s]] == epoch, which the parent's
      whole item, or the chunk item of the parent whose arrival comes last,
      publishes.  So every item of the parent must come before every item of
      s.  (The chunks of s meet in cnt[s]; none waits for another.)
  Both read the update values of the range at ybase[s] + i and z at zbase[s] /
  zpi[c]: slices of their own 128-byte lines (16 doubles), nobody else's.
  With the deep-tree pre-pass, k_fwd_pre subtracts the values from below the
  range (pre lists) and k_fwd_sf those from inside it (late lists).
The gather (k_update*) has no waits between chunks, but a unit's tile is the
sum over its k-slots: a slot in two chunks or in none is a silently wrong
factor, and the split units' partial tiles and arrival counters are indexed
by ck_part / ck_q.
A substitution sweep launches the two step lists of the schedule in order
(sweep.fwd, sweep.bwd; KktDevice::run_sweep_steps walks them): the rule that
picks a level's kernels, the lists' order and their launch totals are checked
here, the totals also against the counts of the commit before the lists."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "linear-programming-vanderbei_amd"))
import ipo_amd  # noqa: E402
from conftest import mps_path  # noqa: E402

TR = 64                 # kTileRows: rows of a solve chunk, of a panel tile
SLAB = 16               # kSlab
MAX_CHUNK_SLOTS = 512   # kMaxChunkSlots
CHUNK_ROWS = 128        # kChunkRows

NAMES = [
    "plan.dims", "plan.col0", "plan.rowptr", "plan.parent", "plan.level", "plan.level_ptr", "plan.level_sups",
    "plan.sup_of", "plan.yrow_ptr", "plan.yrow_idx", "plan.unit_level_ptr", "plan.unit_sup", "plan.kslot",
    "plan.kslot_ptr", "plan.tail_kslot_ptr", "plan.task_src", "paths",
    "panels.fu_sup", "panels.fu_j", "panels.small_sups", "panels.fu_ptr", "panels.small_ptr", "panels.small1_cnt",
    "chunks.chunk_sup", "chunks.chunk_r0", "chunks.sup_chunk0", "chunks.chunk_ptr", "chunks.dims",
    "order.sweep_sups", "order.leaf_cnt", "order.leaf8_cnt",
    "sf.dims", "sf.ybase", "sf.yrow_idx", "sf.zbase", "sf.zpi", "sf.need", "sf.par", "sf.items_f", "sf.items_b",
    "sf.ylate_ptr", "sf.ylate_idx", "sf.pre_col", "sf.pre_ptr", "sf.pre_idx",
    "visits.kslot", "visits.kptr", "visits.late_b", "visits.vis",
    "gather.ck_u", "gather.ck_b", "gather.ck_e", "gather.ck_part", "gather.ck_q", "gather.sp_u", "gather.sp_p0",
    "gather.sp_n", "gather.ck_ptr", "gather.sp_ptr", "gather.ck_kind", "gather.dims",
    "tail.visit_list", "tail.visit_ptr", "tail.run_items", "tail.run_ptr",
    "sweep.fwd", "sweep.bwd", "sweep.fwd_blocked", "sweep.bwd_blocked", "work.launches",
]
# SweepKind (kkt_schedule.h); a step is (kind, q0, n, a, b)
(CHUNKED, PLAIN, LEAF8, MERGED, LEAF, PRE, SYNC_FREE, TAIL_GATHER, TAIL_LEAD, TAIL_CHAIN, TAIL_PAIR, TAIL_BLOCK,
 TAIL_DSCALE) = range(13)
LEVEL_KINDS = (CHUNKED, PLAIN, LEAF8, MERGED, LEAF)
# the knobs the sweeps' step lists depend on
SWEEP_KNOBS = ("IPO_HIP_VISITS", "IPO_HIP_MERGE_LEVELS", "IPO_HIP_SMALL_LEAVES", "IPO_HIP_SF", "IPO_HIP_CHAIN_PAIRS",
               "IPO_HIP_CHAIN_LEAD")


class Sched:
    def __init__(self, name, cus):
        p = ipo_amd.load_mps(mps_path(name))
        d = ipo_amd.kkt_schedule(p.m, p.n, p.kA, p.iA, NAMES, cus=cus)
        self.a = {k: v.astype(np.int64) for k, v in d.items()}
        self.T, self.nsup, self.nlevels, self.tail_c0, self.nt, self.ntb = (int(x) for x in self.a["plan.dims"])
        (self.visits, self.chain_lead, _, _, self.small_leaves, _) = (int(x) for x in self.a["paths"])
        self.sf_level, self.ybuf_stride, self.zpad_stride, self.late_lists = (int(x) for x in self.a["sf.dims"])
        self.nc = np.diff(self.a["plan.col0"])
        self.hb = np.diff(self.a["plan.rowptr"])

    def __getitem__(self, k):
        return self.a[k]

    def in_range(self):
        return self["plan.level"] >= self.sf_level

    def chunked_level(self, l):
        cp = self["chunks.chunk_ptr"]
        return cp[l + 1] > cp[l]

    def src_of_yentry(self, idx):
        """supernode whose row set holds entry idx of the plan's update values"""
        return np.searchsorted(self["plan.rowptr"], idx, side="right") - 1


def load_env(name, cus, env, monkeypatch):
    """the schedule with exactly the knobs of env set among SWEEP_KNOBS"""
    for k in SWEEP_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return Sched(name, cus)


def load(name, cus, visits, monkeypatch):
    return load_env(name, cus, {"IPO_HIP_VISITS": "1"} if visits else {}, monkeypatch)


# ------------------------------------------------------------ sync-free plan
def item_lists(S, key):
    it = S[key].reshape(-1, 2)
    per = {}
    for i, (s, code) in enumerate(it.tolist()):
        per.setdefault(s, []).append((i, code))
    return it, per


def check_sync_free(S):
    level, parent = S["plan.level"], S["plan.parent"]
    rng = S.in_range()
    ns = S.nsup
    fwd, fper = item_lists(S, "sf.items_f")
    bwd, bper = item_lists(S, "sf.items_b")
    c0, csup, cr0 = S["chunks.sup_chunk0"], S["chunks.chunk_sup"], S["chunks.chunk_r0"]
    members = set(np.flatnonzero(rng).tolist())
    for per in (fper, bper):
        assert set(per) == members, "exactly the supernodes of the range"
        for s, lst in per.items():
            codes = [c for _, c in lst]
            if codes == [-1]:
                assert not S.chunked_level(level[s]), s
                continue
            nch = (int(S.hb[s]) + TR - 1) // TR
            assert S.chunked_level(level[s]) and nch >= 1, s
            assert codes == list(range(int(c0[s]), int(c0[s]) + nch)), (s, codes)
            for c, code in enumerate(codes):
                assert csup[code] == s and cr0[code] == TR * c, (s, code)
    # order: children before parents forward, parents before children backward
    need = np.zeros(ns, np.int64)
    for s in members:
        pa = int(parent[s])
        if pa < 0:
            continue
        assert level[pa] > level[s] and pa in members, (s, pa)
        assert max(i for i, _ in fper[s]) < min(i for i, _ in fper[pa]), ("forward", s, pa)
        assert max(i for i, _ in bper[pa]) < min(i for i, _ in bper[s]), ("backward", s, pa)
        need[pa] += len(fper[s])
    assert np.array_equal(S["sf.need"], need)
    assert np.array_equal(S["sf.par"], np.where(rng, parent, -1))
    # padded slices of the update values
    rowptr, ybase = S["plan.rowptr"], S["sf.ybase"]
    assert np.array_equal(ybase[:ns][~rng], rowptr[:ns][~rng])
    yb = ybase[:ns][rng]
    assert np.all(yb % 16 == 0) and np.all(yb >= rowptr[-1])
    o = np.argsort(yb, kind="stable")
    assert np.all(yb[o][1:] >= (yb + S.hb[rng])[o][:-1]), "ybuf slices overlap"
    assert np.all(yb + S.hb[rng] <= ybase[ns]) and ybase[ns] <= S.ybuf_stride
    # padded z slices
    col0, zbase, zpi = S["plan.col0"], S["sf.zbase"], S["sf.zpi"]
    assert np.all(zbase[~rng] == -1)
    zb = zbase[rng]
    assert np.all(zb % 16 == 0) and np.all(zb >= 0)
    o = np.argsort(zb, kind="stable")
    assert np.all(zb[o][1:] >= (zb + S.nc[rng])[o][:-1]), "zpad slices overlap"
    assert np.all(zb + S.nc[rng] <= S.zpad_stride)
    want = np.full(max(S.T, 1), -1, np.int64)
    for s in members:
        want[col0[s]:col0[s + 1]] = zbase[s] + np.arange(S.nc[s])
    assert np.array_equal(zpi, want)
    # the update lists through the new positions
    pidx = S["plan.yrow_idx"]
    src = S.src_of_yentry(pidx)
    assert np.array_equal(S["sf.yrow_idx"], ybase[src] + (pidx - rowptr[src]))
    return len(fwd), len(bwd)


def check_late_and_pre(S):
    """visits on: late + pre lists partition each range column's update list by where the source lies"""
    assert S.late_lists == 1
    level, sup_of, yp = S["plan.level"], S["plan.sup_of"], S["plan.yrow_ptr"]
    early = level[S.src_of_yentry(S["plan.yrow_idx"])] < S.sf_level
    full = S["sf.yrow_idx"]
    lptr, lidx = S["sf.ylate_ptr"], S["sf.ylate_idx"]
    pcol, pptr, pidx = S["sf.pre_col"], S["sf.pre_ptr"], S["sf.pre_idx"]
    assert len(lptr) == S.T + 1 and lptr[0] == 0 and lptr[-1] == len(lidx)
    assert len(pptr) == len(pcol) + 1 and pptr[0] == 0 and pptr[-1] == len(pidx)
    assert np.all(np.diff(pcol) > 0)
    pre_of = {int(c): j for j, c in enumerate(pcol)}
    for v in range(S.T):
        in_rng = v < S.tail_c0 and level[sup_of[v]] >= S.sf_level
        late = lidx[lptr[v]:lptr[v + 1]]
        if not in_rng:
            assert len(late) == 0 and v not in pre_of, v
            continue
        e = slice(yp[v], yp[v + 1])
        assert np.array_equal(late, full[e][~early[e]]), v
        j = pre_of.get(v)
        pre = pidx[pptr[j]:pptr[j + 1]] if j is not None else pidx[:0]
        assert np.array_equal(pre, full[e][early[e]]), v
        assert (j is not None) == bool(early[e].any()), v
    return len(pcol)


# ------------------------------------------------------------- gather chunks
def check_gather(S):
    L = S.nlevels
    ck_ptr, sp_ptr, kind = S["gather.ck_ptr"], S["gather.sp_ptr"], S["gather.ck_kind"]
    cu, cb, ce, cp, cq = (S["gather.ck_" + k] for k in ("u", "b", "e", "part", "q"))
    su, sp0, sn = S["gather.sp_u"], S["gather.sp_p0"], S["gather.sp_n"]
    assert len(ck_ptr) == L + 2 and len(sp_ptr) == L + 2 and len(kind) == L + 1
    assert ck_ptr[-1] == len(cu) and sp_ptr[-1] == len(su)
    vis = S["visits.vis"].reshape(-1, 4)
    ulp, kp, tp = S["plan.unit_level_ptr"], S["plan.kslot_ptr"], S["plan.tail_kslot_ptr"]
    max_np = 0
    for g in range(L + 1):
        chunks = list(range(int(ck_ptr[g]), int(ck_ptr[g + 1])))
        gv = [tuple(r[1:]) for r in vis.tolist() if r[0] == g]
        if g == 0:
            assert not chunks and not gv
            continue
        if g < L:
            units = range(int(ulp[g]), int(ulp[g + 1]))
            rng = ((lambda u: (int(S["visits.late_b"][u]), int(S["visits.kptr"][u + 1]))) if S.visits else
                   (lambda u: (int(kp[u]), int(kp[u + 1]))))
        else:
            units = range(S.ntb * (S.ntb + 1) // 2) if S.nt > 0 else range(0)
            rng = lambda u: (int(tp[u]), int(tp[u + 1]))     # noqa: E731
        live = [(u,) + rng(u) for u in units if rng(u)[1] > rng(u)[0]]
        if kind[g] == 2:        # quadrant gathers: every unit and visit whole, once per quadrant it holds
            got = {}
            for i in chunks:
                assert -4 <= cp[i] <= -1 and cq[i] == -1
                got.setdefault((int(cu[i]), int(cb[i]), int(ce[i])), []).append(int(cp[i]))
            assert set(got) == set(live) | set(gv), g
            assert len(live) + len(gv) == len(set(live) | set(gv))
            assert all(len(q) == len(set(q)) for q in got.values())
            assert sp_ptr[g + 1] == sp_ptr[g]
            continue
        # the group's visits close it, in their order, unsplit
        nv = len(gv)
        tail = chunks[len(chunks) - nv:]
        assert [(int(cu[i]), int(cb[i]), int(ce[i])) for i in tail] == gv, g
        assert all(cp[i] == -1 and cq[i] == -1 for i in tail)
        i = int(ck_ptr[g])
        npart, q = 0, int(sp_ptr[g])
        for u, kb, ke in live:
            first = i
            pos = kb
            while i < ck_ptr[g + 1] - nv and cu[i] == u and pos < ke:
                assert cb[i] == pos and cb[i] < ce[i] <= ke and ce[i] - cb[i] <= MAX_CHUNK_SLOTS, (g, u, i)
                pos = int(ce[i])
                i += 1
            assert pos == ke, ("unit not covered", g, u)
            nch = i - first
            if nch == 1:
                assert cp[first] == -1 and cq[first] == -1
            else:
                assert list(cp[first:i]) == list(range(npart, npart + nch)), (g, u)
                assert np.all(cq[first:i] == q) and su[q] == u and sp0[q] == npart and sn[q] == nch, (g, u)
                npart += nch
                q += 1
        assert i == ck_ptr[g + 1] - nv and q == sp_ptr[g + 1], g
        max_np = max(max_np, npart)
    split_cnt, partial_tiles = (int(x) for x in S["gather.dims"])
    assert split_cnt >= max(1, len(su)) and partial_tiles >= max(1, max_np)
    return len(su)


def check_visits(S):
    """visits on: per unit, the late range and the visits tile the reordered slots exactly once"""
    level, usup, src = S["plan.level"], S["plan.unit_sup"], S["plan.task_src"]
    kslot, kptr, late_b = S["visits.kslot"], S["visits.kptr"], S["visits.late_b"]
    pk, pkp, ulp = S["plan.kslot"], S["plan.kslot_ptr"], S["plan.unit_level_ptr"]
    vis = S["visits.vis"].reshape(-1, 4)
    by_unit = {}
    for g, u, b, e in vis.tolist():
        by_unit.setdefault(u, []).append((b, e, g))
        lu = level[usup[u]]
        assert 1 <= g < lu, ("a visit below its unit's level", g, u)
        k = kslot[b:e]
        k = k[k >= 0]
        assert len(k) > 0 and np.all(level[src[k >> 6]] < g), ("visit sources below the group", g, u)
    assert np.all(kptr[:ulp[1] + 1] == 0)
    for u in range(int(ulp[1]), len(usup)):
        b, e = int(kptr[u]), int(kptr[u + 1])
        assert (e - b) % SLAB == 0 and b <= late_b[u] <= e
        k = kslot[b:e]
        p = pk[pkp[u]:pkp[u + 1]]
        assert np.array_equal(np.sort(k[k >= 0]), np.sort(p[p >= 0])), u
        assert np.all(k[:np.count_nonzero(k >= 0)] >= 0), "padding last"
        pos = b
        for vb, ve, _ in sorted(by_unit.get(u, [])):
            assert vb == pos and ve > vb, u
            pos = ve
        assert pos == late_b[u], u
        gs = [g for _, _, g in sorted(by_unit.get(u, []))]
        assert gs == sorted(set(gs)), ("one visit per unit per launch, in slot order", u)
    return len(vis)


# ------------------------------------------------ cheap structural invariants
def check_structure(S):
    lp, ls = S["plan.level_ptr"], S["plan.level_sups"]
    fu_ptr, sm_ptr = S["panels.fu_ptr"], S["panels.small_ptr"]
    fs, fj, ss, s1 = S["panels.fu_sup"], S["panels.fu_j"], S["panels.small_sups"], S["panels.small1_cnt"]
    h = S.nc + S.hb
    cp, csup, cr0, c0 = (S["chunks." + k] for k in ("chunk_ptr", "chunk_sup", "chunk_r0", "sup_chunk0"))
    sw, nl, n8 = S["order.sweep_sups"], S["order.leaf_cnt"], S["order.leaf8_cnt"]
    ylen = np.diff(S["plan.yrow_ptr"])
    chunked_sups = set()
    for l in range(S.nlevels):
        sups = ls[lp[l]:lp[l + 1]]
        f = slice(fu_ptr[l], fu_ptr[l + 1])
        small = ss[sm_ptr[l]:sm_ptr[l + 1]]
        fused = []
        i = int(fu_ptr[l])
        while i < fu_ptr[l + 1]:
            sp = int(fs[i])
            nw = max(1, (int(h[sp]) + TR - 1) // TR - 1)
            assert list(fj[i:i + nw]) == list(range(nw)) and np.all(fs[i:i + nw] == sp), (l, sp)
            fused.append(sp)
            i += nw
        assert i == fu_ptr[l + 1] and len(fs[f]) == i - fu_ptr[l]
        assert sorted(fused + small.tolist()) == sorted(sups.tolist()), l
        assert np.all((S.nc[small] <= 16) & (h[small] <= TR)) and not np.any((S.nc[fused] <= 16) & (h[fused] <= TR))
        one = (S.nc[small] == 1) & (h[small] <= 8)
        assert np.all(one[:s1[l]]) and (s1[l] == 0 or (s1[l] >= S.small_leaves and not np.any(one[s1[l]:])))
        # solve chunks
        big = bool(np.any(S.hb[sups] > CHUNK_ROWS))
        assert big == (cp[l + 1] > cp[l]), l
        order = sw[lp[l]:lp[l + 1]]
        if big:
            pos = int(cp[l])
            for sp in sups.tolist():
                assert c0[sp] == pos
                r = list(range(0, int(S.hb[sp]), TR))
                assert list(cr0[pos:pos + len(r)]) == r and np.all(csup[pos:pos + len(r)] == sp), sp
                pos += len(r)
                chunked_sups.add(sp)
            assert pos == cp[l + 1]
            assert np.array_equal(order, sups) and nl[l] == 0 and n8[l] == 0
            continue
        # sweep order: leaves first, the small ones first among them
        assert sorted(order.tolist()) == sorted(sups.tolist()), l
        leaf = (S.nc[order] == 1) & (S.hb[order] <= 64)
        assert np.all(leaf[:nl[l]]) and not np.any(leaf[nl[l]:]), l
        c = S["plan.col0"][order]
        small8 = leaf & (S.hb[order] <= 8) & (ylen[c] <= 8)
        assert n8[l] <= nl[l] and np.all(small8[:n8[l]])
        assert n8[l] == 0 or (n8[l] >= S.small_leaves and not np.any(small8[n8[l]:nl[l]]))
    assert np.all(c0[[s for s in range(S.nsup) if s not in chunked_sups]] == -1)
    assert int(S["chunks.dims"][0]) == max(1, len(csup) * 64)


def check_tail_lists(S, cus):
    """the dense tail's lists (their order: test_tail_schedule.py) belong to this plan's tail"""
    vl, vp, ri, rp = (S["tail." + k] for k in ("visit_list", "visit_ptr", "run_items", "run_ptr"))
    if S.nt == 0:
        assert len(vl) == len(vp) == len(ri) == len(rp) == 0
        return
    gp = [max(1, (S.nt - t * 64 + TR - 1) // TR - 1) for t in range(S.ntb)]
    assert len(vp) == S.ntb + 1 and vp[0] == 0 and vp[-1] == len(vl) and np.all(np.diff(vp) >= 0)
    assert len(rp) == S.ntb + 1 and rp[0] == 0 and 2 * rp[-1] == len(ri) and np.all(np.diff(rp) >= 0)
    y = ri.reshape(-1, 2)[:, 1] & 0xffffffff
    assert np.count_nonzero(y >> 31) == sum(gp), "every panel workgroup once"
    assert len(y) - sum(gp) == len(vl) or cus < 256, "the run's visits are the steps' at equal chunks"


# ------------------------------------------------------- the sweeps' step lists
def steps_of(S, key):
    return [tuple(r) for r in S[key].reshape(-1, 5).tolist()]


def launches(steps):
    return sum(2 if st[0] == CHUNKED else 1 for st in steps)


def by_level(S, steps):
    """consecutive level steps grouped by the level their q0 lies in: [(level, [steps])]"""
    lp = S["plan.level_ptr"]
    out = []
    for st in steps:
        assert st[0] in LEVEL_KINDS, st
        l = int(np.searchsorted(lp, st[1], side="right")) - 1
        if not out or out[-1][0] != l:
            out.append((l, []))
        out[-1][1].append(st)
    return out


def check_sweep_steps(S, merge=True, pairs=False):
    """sweep.fwd / sweep.bwd: the rule of every level, the order of the lists, their totals"""
    lp, cp = S["plan.level_ptr"], S["chunks.chunk_ptr"]
    nl, n8 = S["order.leaf_cnt"], S["order.leaf8_cnt"]
    fwd, bwd = steps_of(S, "sweep.fwd"), steps_of(S, "sweep.bwd")
    nlev_f = next((i for i, st in enumerate(fwd) if st[0] not in LEVEL_KINDS), len(fwd))
    head_b = next((i for i, st in enumerate(bwd) if st[0] in LEVEL_KINDS), len(bwd))
    lev_f, lev_b = by_level(S, fwd[:nlev_f]), by_level(S, bwd[head_b:])
    # levels [0, sf_level) ascending / descending, a level's steps the same in both
    assert [l for l, _ in lev_f] == list(range(S.sf_level))
    assert lev_b == lev_f[::-1]
    for l, steps in lev_f:
        q0, q1 = int(lp[l]), int(lp[l + 1])
        # the ranges partition the level in order
        pos = q0
        for kind, q, n, a, b in steps:
            assert q == pos and n > 0, (l, steps)
            pos += n + (a if kind == MERGED else 0)
        assert pos == q1, (l, steps)
        assert (sum(st[0] == CHUNKED for st in steps) == 1) == bool(S.chunked_level(l)), (l, steps)
        if S.chunked_level(l):
            assert steps == [(CHUNKED, q0, q1 - q0, int(cp[l]), int(cp[l + 1] - cp[l]))], (l, steps)
            continue
        k, k8 = int(nl[l]), int(n8[l])
        want = [(LEAF8, q0, k8, 0, 0)] if k8 > 0 else []
        if merge and k > k8 and q1 - q0 > k:
            want.append((MERGED, q0 + k8, k - k8, q1 - q0 - k, 0))
        else:
            if k > k8:
                want.append((LEAF, q0 + k8, k - k8, 0, 0))
            if q1 - q0 > k:
                want.append((PLAIN, q0 + k, q1 - q0 - k, 0, 0))
        assert steps == want, (l, steps, want)
    # after the forward levels: pre-pass and sync-free range, then the tail; mirrored backward
    npre, late = len(S["sf.pre_col"]), int(late_lists_read(S))
    rng = S.sf_level < S.nlevels
    want_f = [(PRE, 0, npre, 0, 0)] if npre > 0 else []
    want_b = []
    if S.nt > 0:
        want_b.append((TAIL_PAIR if pairs else TAIL_CHAIN, 0, 0, 0, 0))
    if rng:
        want_f.append((SYNC_FREE, 0, len(S["sf.items_f"]) // 2, late, 0))
        want_b.append((SYNC_FREE, 0, len(S["sf.items_b"]) // 2, 0, 0))
    if S.nt > 0:
        want_f += [(TAIL_GATHER, 0, 0, 0, 0), (TAIL_LEAD if S.chain_lead else TAIL_CHAIN, 0, 0, 0, 0)]
    assert not npre or rng, "a pre-pass without a range"
    assert fwd[nlev_f:] == want_f, (fwd[nlev_f:], want_f)
    assert bwd[:head_b] == want_b, (bwd[:head_b], want_b)
    assert list(S["work.launches"]) == [launches(fwd), launches(bwd)]


def late_lists_read(S):
    """the forward sync-free launch reads the late lists"""
    return len(S["sf.pre_col"]) > 0 or S.late_lists == 1


def check_blocked_steps(S):
    """sweep.*_blocked: the blocked tail's rule applied to this plan"""
    lp, cp = S["plan.level_ptr"], S["chunks.chunk_ptr"]
    fwd, bwd = steps_of(S, "sweep.fwd_blocked"), steps_of(S, "sweep.bwd_blocked")
    levels = [(CHUNKED, int(lp[l]), int(lp[l + 1] - lp[l]), int(cp[l]), int(cp[l + 1] - cp[l])) if S.chunked_level(l)
              else (PLAIN, int(lp[l]), int(lp[l + 1] - lp[l]), 0, 0) for l in range(S.nlevels)]
    assert S.ntb >= 2
    blocks = [(TAIL_BLOCK, 0, 0, kb, 0) for kb in range(S.ntb)]
    assert fwd == levels + [(TAIL_GATHER, 0, 0, 0, 0)] + blocks
    assert bwd == [(TAIL_DSCALE, 0, 0, 0, 0)] + blocks[::-1] + levels[::-1]
    assert not any(st[0] in (SYNC_FREE, PRE) for st in fwd + bwd)


def chunked_levels_in_range(S):
    return sum(bool(S.chunked_level(l)) for l in range(S.sf_level, S.nlevels))


# what each problem is here for (the figures hold at the default knobs)
CASES = {
    # the whole tree is the sync-free range; no tail
    "afiro": lambda S, nsplit: S.sf_level == 0 and S.nlevels >= 2 and S.nt == 0,
    # range from level 1, one chunked level inside it, a tail of 7 block columns
    "25fv47": lambda S, nsplit: S.sf_level == 1 and chunked_levels_in_range(S) == 1 and S.ntb == 7,
    # range from level 5, 5 chunked levels inside it, split-K happens
    "pds-02": lambda S, nsplit: S.sf_level == 5 and chunked_levels_in_range(S) == 5 and nsplit >= 1,
    # range from level 7, 13 chunked levels, a tail of 70 block columns
    "dfl001": lambda S, nsplit: S.sf_level == 7 and chunked_levels_in_range(S) == 13 and S.ntb == 70,
    # no tail; split units
    "ken-07": lambda S, nsplit: S.nt == 0 and S.sf_level < S.nlevels and nsplit >= 1,
}


@pytest.mark.parametrize("cus", [256, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_schedule(name, cus, monkeypatch):
    S = load(name, cus, False, monkeypatch)
    assert S.visits == 0 and S.late_lists == 0 and len(S["visits.vis"]) == 0 and len(S["sf.pre_col"]) == 0
    nf, nb = check_sync_free(S)
    assert nf > 0 and nb > 0 and S.sf_level < S.nlevels, "a range exists"
    nsplit = check_gather(S)
    check_structure(S)
    check_tail_lists(S, cus)
    check_sweep_steps(S)
    assert CASES[name](S, nsplit), (name, S.sf_level, chunked_levels_in_range(S), S.ntb, nsplit)


@pytest.mark.parametrize("name", ["25fv47", "pds-02"])
def test_schedule_with_visits(name, monkeypatch):
    """IPO_HIP_VISITS=1: the deep-tree gather visits and the sweeps' pre-pass on trees that would not get them"""
    S = load(name, 256, True, monkeypatch)
    assert S.visits == 1
    nf, nb = check_sync_free(S)
    assert nf > 0 and nb > 0
    assert check_late_and_pre(S) >= 1, "a pre-pass column"
    assert check_visits(S) >= 1, "a visit"
    check_gather(S)
    check_structure(S)
    check_sweep_steps(S)
    # k_fwd_pre is counted where it runs; the commit before the lists launched it uncounted
    pf, pb = PARENT_LAUNCHES_VISITS[name]
    assert list(S["work.launches"]) == [pf + (1 if len(S["sf.pre_col"]) else 0), pb]


# work.launches (forward, backward) of the commit before the step lists, whose
# count_work restated the launch rule as arithmetic: recorded from a build of
# that commit, not from the code under test.  The lists must total the same.
PARENT_LAUNCHES = {
    "default": ({}, {"afiro": (1, 1), "25fv47": (4, 3), "pds-02": (8, 7), "dfl001": (10, 9), "ken-07": (5, 5)}),
    "merge0": ({"IPO_HIP_MERGE_LEVELS": "0"},
               {"afiro": (1, 1), "25fv47": (4, 3), "pds-02": (12, 11), "dfl001": (16, 15), "ken-07": (8, 8)}),
    "small1": ({"IPO_HIP_SMALL_LEAVES": "1"},
               {"afiro": (1, 1), "25fv47": (5, 4), "pds-02": (13, 12), "dfl001": (16, 15), "ken-07": (8, 8)}),
    "sf0": ({"IPO_HIP_SF": "0"},
            {"afiro": (7, 7), "25fv47": (24, 23), "pds-02": (26, 25), "dfl001": (35, 34), "ken-07": (17, 17)}),
}
# the same with IPO_HIP_VISITS=1 (that commit did not count k_fwd_pre)
PARENT_LAUNCHES_VISITS = {"25fv47": (4, 3), "pds-02": (8, 7)}


@pytest.mark.parametrize("setting", list(PARENT_LAUNCHES))
@pytest.mark.parametrize("name", list(CASES))
def test_sweep_steps_total_the_parents_launches(name, setting, monkeypatch):
    env, want = PARENT_LAUNCHES[setting]
    S = load_env(name, 256, env, monkeypatch)
    check_structure(S)
    check_sweep_steps(S, merge=setting != "merge0")
    assert tuple(int(x) for x in S["work.launches"]) == want[name]
    kinds = {st[0] for st in steps_of(S, "sweep.fwd")}
    assert setting != "sf0" or (SYNC_FREE not in kinds and S.sf_level == S.nlevels)


def test_sweep_steps_see_every_level_kind(monkeypatch):
    """between them the settings above reach every level kind (so the rule's branches are all checked)"""
    seen = set()
    for setting, name in (("sf0", "dfl001"), ("merge0", "pds-02"), ("small1", "pds-02")):
        S = load_env(name, 256, PARENT_LAUNCHES[setting][0], monkeypatch)
        seen |= {st[0] for st in steps_of(S, "sweep.fwd")}
    assert seen >= set(LEVEL_KINDS), seen


@pytest.mark.parametrize("env,pairs,lead", [({"IPO_HIP_CHAIN_PAIRS": "1"}, True, 1),
                                            ({"IPO_HIP_CHAIN_LEAD": "0"}, False, 0)])
def test_sweep_steps_tail_knobs(env, pairs, lead, monkeypatch):
    S = load_env("25fv47", 256, env, monkeypatch)
    assert S.nt > 0 and S.chain_lead == lead
    check_sweep_steps(S, pairs=pairs)


@pytest.mark.parametrize("name", ["dfl001", "25fv47"])
def test_sweep_steps_blocked(name, monkeypatch):
    """No committed problem has a tail of more than kChainMaxBlocks block columns: the builder's rule for one,
    forced on here"""
    check_blocked_steps(load_env(name, 256, {}, monkeypatch))


def test_unknown_array_is_an_error():
    p = ipo_amd.load_mps(mps_path("afiro"))
    with pytest.raises(ipo_amd.IpoHipError, match="unknown array"):
        ipo_amd.kkt_schedule(p.m, p.n, p.kA, p.iA, "sf.nope")
    one = ipo_amd.kkt_schedule(p.m, p.n, p.kA, p.iA, "plan.dims")
    assert list(one) == list(ipo_amd.kkt_schedule(p.m, p.n, p.kA, p.iA, ["plan.dims", "paths"])["plan.dims"])
