"""Host-side walk over every global row that the ragged attention kernels
(csrc/kernels/attention.hip, TAIL variants) read or write, with the kernels'
own index expressions: staged chunks (Stage::fetch / fetch_rows), pinned
fragments, lse/delta traffic and the epilogue rows. For every (NW, T):

  - no access touches a row >= T of its (batch, head);
  - every row < T of o/dq/dk/dv, lse and delta is written exactly once;
  - every tile that a loop stages delivers all of its rows < T.

--D 128 walks the tail kernels of csrc/kernels/attention_d128.hip instead:
two-image tiles whose row count next_tiles128 steps, the 2-wave dkv kernel's
own K and V tile (stage_tile128_scaled) and 256-byte epilogue rows
(store_ctiles128).

Run it before the first GPU run of a change to those predicates:
    python scripts/attn_ragged_bounds.py [--D 64|128] [T ...]
"""

import argparse

KVB = 64
DEFAULT_T = (1, 37, 63, 65, 96, 127, 129, 200, 255, 257, 300, 1000)


def nw_rule(T, knob=8):
    """attn_dispatch: the widest block that divides T rounded up to 64."""
    t64 = (T + KVB - 1) // KVB * KVB
    if t64 % 256 == 0 and knob == 8:
        return 8
    if t64 % 128 == 0 and knob >= 4:
        return 4
    return 2


def staged_rows(tid, nt, left):
    """Tile rows whose chunk thread `tid` reads: TilePipe::fetch."""
    rows = []
    for rep in range(512 // nt):
        r = (tid + rep * nt) >> 3
        if left >= KVB or r < left:      # fetch() / fetch_rows()
            rows.append(r)
    return rows


def epilogue_rows(lane, rows_valid):
    """store_ctiles<TAIL>: the wave rows this lane stores a piece of."""
    return [8 * i + (lane >> 3) for i in range(4)
            if 8 * i + (lane >> 3) < rows_valid]


def walk(T, nw):
    bm, nt = nw * 32, nw * 64
    n_tiles = (T + bm - 1) // bm
    reads, written = [], {"o": [], "lse": [], "delta": [], "dkv": []}
    for tile in range(n_tiles):
        # ---- forward and dq: a Q block against K/V tiles 0 .. n_kv-1
        n_kv = (tile + 1) * bm // KVB
        for j in range(n_kv):
            left = T - j * KVB
            got = sorted(r for tid in range(nt)
                         for r in staged_rows(tid, nt, left))
            want = sorted(list(range(min(KVB, max(left, 0)))) * 8)
            assert got == want, ("K/V tile", T, nw, tile, j)
            reads += [j * KVB + r for r in got]
        for tid in range(nt):
            lane, w = tid & 63, tid >> 6
            row_lo = tile * bm + w * 32
            row_me = row_lo + (lane & 31)
            if row_me < T:               # q/do/o fragments, lse, delta
                reads.append(row_me)
                if lane < 32:
                    written["lse"].append(row_me)
                    written["delta"].append(row_me)
            if lane & 7 == 0:            # one piece per stored row
                written["o"] += [row_lo + r
                                 for r in epilogue_rows(lane, T - row_lo)]
        # ---- dkv: a key block against Q/dO tiles i0 .. n_q-1
        i0 = tile * bm // KVB
        n_q = (T + KVB - 1) // KVB
        left = T - i0 * KVB
        for i in range(i0, n_q):
            assert left == T - i * KVB and left >= 1
            got = sorted(r for tid in range(nt)
                         for r in staged_rows(tid, nt, left))
            assert got == sorted(list(range(min(KVB, left))) * 8)
            reads += [i * KVB + r for r in got]
            reads += [i * KVB + tid for tid in range(KVB) if tid < left]
            left -= KVB
        for tid in range(nt):
            lane, w = tid & 63, tid >> 6
            key_lo = tile * bm + w * 32
            if key_lo + (lane & 31) < T:
                reads.append(key_lo + (lane & 31))
            if lane & 7 == 0:
                written["dkv"] += [key_lo + r
                                   for r in epilogue_rows(lane, T - key_lo)]
    assert reads and max(reads) < T and min(reads) >= 0, (T, nw, max(reads))
    for name, rows in written.items():
        assert sorted(rows) == list(range(T)), (name, T, nw)


def nw_rule_d128(T):
    """d128_dispatch: 4 waves where 128 divides T rounded up to 64, else 2."""
    return 4 if (T + KVB - 1) // KVB * KVB % 128 == 0 else 2


def epilogue_rows_d128(lane, rows_valid):
    """store_ctiles128<TAIL>: the wave rows this lane stores a piece of."""
    return [4 * i + (lane >> 4) for i in range(8)
            if 4 * i + (lane >> 4) < rows_valid]


class Pipe128:
    """tile128_pipe + next_tiles128: two stages (the halves of the same 64
    rows) under one row count, which next_tiles128 steps before a fetch."""

    def __init__(self, nt, row0, left):
        self.nt, self.row0, self.left = nt, row0, left

    def fetch(self):
        """Global rows read, one entry per 16-byte chunk of both halves."""
        rows = sorted(r for tid in range(self.nt)
                      for r in staged_rows(tid, self.nt, self.left)) * 2
        want = list(range(min(KVB, max(self.left, 0)))) * 16
        assert sorted(rows) == sorted(want), ("tile", self.row0, self.left)
        return [self.row0 + r for r in rows]

    def step(self):
        self.row0 += KVB     # Stage::advance
        self.left -= KVB     # next_tiles128, if constexpr (TAIL)


def walk_d128(T, nw):
    bm, nt = nw * 32, nw * 64
    n_tiles = (T + bm - 1) // bm
    reads, written = [], {"o": [], "lse": [], "delta": [], "dkv": []}
    for tile in range(n_tiles):
        # ---- forward and dq: K and V pipes from row 0, n_kv tiles
        n_kv = (tile + 1) * bm // KVB
        pipe = Pipe128(nt, 0, T)
        reads += pipe.fetch()                        # prime()
        for j in range(n_kv):
            if j + 1 < n_kv:                         # next_tiles128, more
                pipe.step()
                assert pipe.left == T - (j + 1) * KVB >= 1
                reads += pipe.fetch()
        for tid in range(nt):
            lane, w = tid & 63, tid >> 6
            row_lo = tile * bm + w * 32
            row_me = row_lo + (lane & 31)
            if row_me < T:               # q/do/o fragments, lse, delta
                reads.append(row_me)
                if lane < 32:
                    written["lse"].append(row_me)
                    written["delta"].append(row_me)
            if lane & 15 == 0:           # one piece per stored row
                written["o"] += [row_lo + r for r in
                                 epilogue_rows_d128(lane, T - row_lo)]
        # ---- dkv: Q and dO pipes (and lse/delta rows) from tile i0 on
        i0 = tile * bm // KVB
        n_q = (T + KVB - 1) // KVB
        pipe = Pipe128(nt, i0 * KVB, T - i0 * KVB)
        row_left = T - i0 * KVB                      # RowPipe<true>
        assert pipe.left >= 1
        reads += pipe.fetch()
        reads += [i0 * KVB + tid for tid in range(KVB) if tid < row_left]
        for i in range(i0, n_q):
            if i + 1 < n_q:
                pipe.step()
                row_left -= KVB
                assert pipe.left == row_left == T - (i + 1) * KVB >= 1
                reads += pipe.fetch()
                reads += [(i + 1) * KVB + tid for tid in range(KVB)
                          if tid < row_left]
        if nw == 2:
            # stage_tile128_scaled<NT, true>: the block's own K and V tile
            rows_own = T - tile * bm
            got = [chunk >> 4 for chunk in range(1024)
                   if (chunk >> 4) < rows_own]
            assert sorted(set(got)) == list(range(min(KVB, rows_own)))
            reads += [tile * bm + r for r in got]
        for tid in range(nt):
            lane, w = tid & 63, tid >> 6
            key_lo = tile * bm + w * 32
            if nw != 2 and key_lo + (lane & 31) < T:     # pinned K, V
                reads.append(key_lo + (lane & 31))
            if lane & 15 == 0:
                written["dkv"] += [key_lo + r for r in
                                   epilogue_rows_d128(lane, T - key_lo)]
    assert reads and max(reads) < T and min(reads) >= 0, (T, nw, max(reads))
    for name, rows in written.items():
        assert sorted(rows) == list(range(T)), (name, T, nw)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--D", type=int, default=64, choices=(64, 128))
    p.add_argument("T", type=int, nargs="*")
    args = p.parse_args()
    for T in args.T or DEFAULT_T:
        if args.D == 128:
            nw = nw_rule_d128(T)
            walk_d128(T, nw)
            print(f"D=128 T={T:5d} NW={nw} "
                  f"blocks={(T + nw * 32 - 1) // (nw * 32)}: ok")
            continue
        for knob in (8, 4, 2):
            nw = nw_rule(T, knob)
            walk(T, nw)
            print(f"T={T:5d} knob={knob} NW={nw} "
                  f"blocks={(T + nw * 32 - 1) // (nw * 32)}: ok")


if __name__ == "__main__":
    main()
