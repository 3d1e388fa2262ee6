"""A plain model of the chunker's bookkeeping between segments (test infrastructure).

The chunk rule is the closed form (oracle/pyref.chunking_closed_form): after a cut at p the next
cut is one past the first j >= p + 701 with s[j] >= M(p), M(p) = max(0, max s[p .. p + 700]) (no 0
floor for the block's first chunk), or p + 1,000,001 when there is none; no cut once the window
passes the block end.  On top of it, from DESIGN.md §6:

  speculate  segment k walks that rule from s_k = k * seg_len as if a cut were there.  Cuts below
             s_{k+1} are its main cuts, later ones overrun cuts.  All segments step together, one
             cut per step, so at its step t (its cut number t, from 0) a segment sees the first
             t + 1 cuts of the next one.  An overrun cut that is one of those (a main cut of the
             next segment) syncs the boundary: (i, j) = (overrun index, index in the next list).
             The boundary fails at an overrun cut seg_len or more past s_{k+1}, at the lane_over-th
             overrun cut, at a cut at or beyond over_lim = s_{k+2} - 64 (while a whole window is
             left), or when a search would go on into a 1-KiB view (views start at p & ~63) that
             begins beyond over_lim; that last cut is not recorded.  A chain that runs out of data
             ends; the last segment always does.
  repair     a failed boundary's chain goes on from its last recorded cut.  Every cut c is looked
             up among the first min(n_main, lookup) cuts of segment c // seg_len (later than k):
             found at jj after n_ext cuts -> jump (jmp, jj, n_ext).  A cut beyond p0 +
             repair_bytes, repair_cuts cuts, or the block end: give-up.
  stitch     from segment 0: a synced boundary goes to k + 1 (k keeps its overrun cuts before the
             shared one, k + 1 starts at j), a jump to k + jmp (k keeps all its cuts and the
             repair's n_ext - 1, the target starts at jj); the path ends at the last segment, at an
             ended chain, or at a give-up, where the sequential rule finishes the block.  The last
             cut is dropped and the block size appended.

The constants are parameters; their defaults are parsed from the constexpr lines of common.hpp and
chunk.hip, as data.  The model is the reference for intermediate state only: final cuts are judged
by the C oracle, pyref and the designed offsets."""
import bisect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 700
MAXLEN = 1_000_000
END, FAIL, JUMP, GIVEUP = -1, -2, -3, -4
CAPPED = "capped"


def parse_constants(*paths):
    """{name: value} of every `constexpr int kName = <int> [<< <int>];` line."""
    out = {}
    for p in paths:
        for name, a, sh in re.findall(r"constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*(?:<<\s*(\d+))?\s*;", open(p).read()):
            out[name] = int(a) << int(sh or 0)
    return out


_CSRC = os.path.join(ROOT, "hdrf_amd", "csrc")
CONSTANTS = parse_constants(os.path.join(_CSRC, "common.hpp"), os.path.join(_CSRC, "chunk.hip"))


def default_params():
    c = CONSTANTS
    return dict(lane_over=c["kLaneOver"], repair_bytes=c["kRepairBytes"], repair_cuts=c["kRepairCuts"], lookup=64,
                over_slack=64, over_lim_delta=0, view=1024, view_align=64)


class Rule:
    """next cut of a block under the closed-form rule, by the positions of its non-negative bytes."""

    def __init__(self, block):
        self.s = np.asarray(block, np.uint8).view(np.int8)
        self.n = len(self.s)
        self.pos = np.flatnonzero(self.s >= 0)
        self.val = self.s[self.pos]
        self.lpos, self.lval = self.pos.tolist(), self.val.tolist()      # scalar lookups: bisect on lists

    def _search(self, lo, lim, m):
        """first j in [lo, lim] with s[j] >= m, or -1"""
        if m < 0:                                           # the first chunk's unfloored threshold: dense
            for a in range(lo, lim + 1, 1 << 16):
                hit = np.flatnonzero(self.s[a:min(a + (1 << 16), lim + 1)] >= m)
                if len(hit):
                    return a + int(hit[0])
            return -1
        lpos, lval = self.lpos, self.lval
        i, n = bisect.bisect_left(lpos, lo), len(lpos)
        for i in range(i, min(i + 8, n)):
            if lval[i] >= m:
                return lpos[i] if lpos[i] <= lim else -1
        i += 1
        step = 64
        while i < n and lpos[i] <= lim:
            hit = np.flatnonzero(self.val[i:i + step] >= m)
            if len(hit):
                j = lpos[i + int(hit[0])]
                return j if j <= lim else -1
            i += step
            step = min(step * 4, 1 << 16)
        return -1

    def next(self, p, first, cap=None, view=1024, view_align=64):
        """-> the cut after p, None when the data ends, CAPPED when the search would enter a view that
        starts beyond cap."""
        n = self.n
        if p + W > n - 1:
            return None
        if first:
            m = int(self.s[p:p + W + 1].max())
        else:
            a = bisect.bisect_left(self.lpos, p)
            b = bisect.bisect_left(self.lpos, p + W + 1, a)
            m = max(0, max(self.lval[a:b])) if b > a else 0
        lim = min(p + MAXLEN, n - 1)
        j = self._search(p + W + 1, lim, m)
        if cap is not None:
            b0 = p & ~(view_align - 1)
            far = j if j >= 0 else lim
            v = (far - b0) // view                          # the last view the search reads
            if v >= 1 and b0 + view * v > cap:
                return CAPPED
        if j >= 0:
            return j + 1
        return p + MAXLEN + 1 if p + MAXLEN <= n - 1 else None


def sequential(rule, p=0, first=True):
    """every cut of the exact chain from p to the block end"""
    out = []
    while True:
        c = rule.next(p, first)
        if c is None:
            return out
        out.append(c)
        p, first = c, False


class Model:
    """All per-segment state of one block; see the module docstring.  Arrays are indexed by segment."""

    def __init__(self, block, seg_len, **params):
        P = default_params()
        assert set(params) <= set(P), set(params) - set(P)
        P.update(params)
        self.P, self.Ls = P, seg_len
        self.rule = R = Rule(block)
        n = self.size = R.n
        self.nseg = nseg = max(1, -(-n // seg_len))
        Ls = seg_len
        # ---- speculate: main cuts first (they depend on nothing else), then the overrun steps
        main, pend = [], []
        for k in range(nseg):
            e = (k + 1) * Ls if k + 1 < nseg else None
            cuts, p, first = [], k * Ls, k == 0
            nxt = None
            while True:
                c = R.next(p, first, cap=self._over_lim(k), view=P["view"], view_align=P["view_align"])
                if c is None or c is CAPPED or (e is not None and c >= e):
                    nxt = c
                    break
                cuts.append(c)
                p, first = c, False
            main.append(cuts)
            pend.append(nxt)
        self.main = main
        self.over = over = [[] for _ in range(nseg)]
        self.sync = sync = np.full(nseg, END, np.int64)
        for k in range(nseg - 1):
            e, lim = (k + 1) * Ls, self._over_lim(k)
            nm = len(main[k])
            c = pend[k]
            p = main[k][-1] if nm else k * Ls
            while True:
                if c is None:
                    break                                   # the data ended: END
                if c is CAPPED:
                    sync[k] = FAIL
                    break
                t = nm + len(over[k])                       # this cut's step
                over[k].append(c)
                rel = c - e
                seen = main[k + 1][:t + 1]
                if rel >= Ls:
                    sync[k] = FAIL
                elif c in seen:
                    sync[k] = (len(over[k]) - 1) | (seen.index(c) << 16)
                elif len(over[k]) >= P["lane_over"]:
                    sync[k] = FAIL
                elif c >= lim and c + W <= n - 1:
                    sync[k] = FAIL
                if sync[k] != END:
                    break
                p = c
                c = R.next(p, False, cap=lim, view=P["view"], view_align=P["view_align"])
        self.n_main = np.array([len(m) for m in main], np.int64)
        self.n_over = np.array([len(o) for o in over], np.int64)
        self.failed = np.flatnonzero(sync == FAIL)
        self.rq_count = len(self.failed)
        # ---- repair
        self.jmp = np.zeros(nseg, np.int64)
        self.jj = np.zeros(nseg, np.int64)
        self.n_ext = np.zeros(nseg, np.int64)
        self.ext = {}                                       # k -> the repair's cuts, the shared one included
        self.repair_span = {}                               # k -> bytes from p0 to the repair's last cut
        for k in self.failed:
            k = int(k)
            cuts = main[k] + over[k]
            p0 = cuts[-1] if cuts else k * Ls
            p, first, walked, status = p0, not cuts and k == 0, [], GIVEUP
            while len(walked) < P["repair_cuts"]:
                c = R.next(p, first)
                if c is None:
                    break
                walked.append(c)
                if c > p0 + P["repair_bytes"]:
                    break
                m = c // Ls
                if k < m < nseg:
                    look = main[m][:P["lookup"]]
                    if c in look:
                        status = JUMP
                        self.jmp[k], self.jj[k], self.n_ext[k] = m - k, look.index(c), len(walked)
                        break
                p, first = c, False
            sync[k] = status
            self.ext[k] = walked
            self.repair_span[k] = (walked[-1] if walked else p0) - p0
        # ---- stitch: the path through the irregular boundaries, the pieces, the fallback
        self.nodes = [int(k) for k in np.flatnonzero(sync[:nseg - 1] < 0)]
        self.on_path = np.zeros(nseg, bool)
        self.piece = np.zeros(nseg, np.int64)
        self.ext_dst = np.full(nseg, -1, np.int64)
        self.jumps = []                                     # on-path (source, target)
        offs, k, frm = [], 0, 0
        self.fallback = False
        while True:
            self.on_path[k] = True
            sy = int(sync[k])
            part = main[k][frm:]
            if k == nseg - 1 or sy in (END, GIVEUP, FAIL):
                part = part + over[k]
                self.term = k
                self.fallback = sy in (GIVEUP, FAIL)
                nxt = None
            elif sy == JUMP:
                part = part + over[k]
                if len(part) + self.n_ext[k] - 1 > 0:
                    self.ext_dst[k] = len(offs) + len(part)
                part = part + self.ext[k][:-1]
                self.jumps.append((k, k + int(self.jmp[k])))
                nxt, nfrm = k + int(self.jmp[k]), int(self.jj[k])
            else:
                part = part + over[k][:sy & 0xffff]
                nxt, nfrm = k + 1, sy >> 16
            self.piece[k] = len(part)
            offs += part
            if nxt is None:
                break
            k, frm = nxt, nfrm
        self.fail_dst = len(offs) if self.fallback else -1
        if self.fallback:
            offs += sequential(R, offs[-1] if offs else 0, not offs)
        assert all(a < b for a, b in zip(offs, offs[1:])), "the model's cuts do not ascend"
        self.n_cuts = len(offs)
        self.offsets = np.array((offs[:-1] if offs else []) + [n], np.uint32)

    def _over_lim(self, k):
        if k + 1 >= self.nseg:
            return None
        return (k + 2) * self.Ls - self.P["over_slack"] + self.P["over_lim_delta"]

    def state(self, k):
        """what the model says of segment k, for messages and for the teeth tests"""
        return (int(self.n_main[k]), int(self.n_over[k]), int(self.sync[k]), int(self.jmp[k]), int(self.jj[k]),
                int(self.n_ext[k]), int(self.ext_dst[k]), int(self.piece[k]))

    def node_index(self, k):
        """position of boundary k in the ordered list of irregular boundaries the stitch follows"""
        return self.nodes.index(k)

    def passed_unseen(self):
        """[(k, i, j)]: overrun cut i of segment k is the next segment's main cut j, but at that step
        the next segment had not made it yet (j > n_main[k] + i): not a sync."""
        out = []
        for k in range(self.nseg - 1):
            nm = len(self.main[k])
            for i, c in enumerate(self.over[k]):
                if c in self.main[k + 1]:
                    j = self.main[k + 1].index(c)
                    if j > nm + i:
                        out.append((k, i, j))
                    break
        return out
