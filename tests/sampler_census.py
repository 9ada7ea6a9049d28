"""What the sampler's interval pre-pass left its evaluator, read back from a stepped `VoxelObject` (developer pointers 7 and 8 of
`ivx_grid_device_ptr`: per-chunk compact program lengths, list counters and lists; the compact programs): per listed chunk the program's
length, its op-code histogram and the evaluation list it is on. A property of the pruning, not of the bytes — the tests use it to show that
a scene reaches the rule it is there for (a poisoned chunk, a dropped first operand, a program of exactly OP_CAP ops, ...) before they hold
the bytes to the oracle. Shared by tests/test_gpu_sampler_programs.py, the witnessed seeds of tests/test_gpu_random_sdf.py,
tests/test_gpu_sampler_long_programs.py and tools/poison_census.py."""
import ctypes as C
from collections import namedtuple

import numpy as np

from impact_amd import capi

OP_CONST, OP_LEAF, OP_SCALE, OP_COMBINE, OP_COMBINE_OUTSIDE, OP_SKIP, OP_NOISE, OP_NOISE_OUTSIDE = range(8)
OP_CAP = 128
OP_OVERFLOW = 0xFFFFFFFF
LISTS = ("0 long", "0 short", "1", "2")  # the one-level class's list front (long programs) and back (short ones), the two-level class, the general class

# prog_len: None for a chunk on the full program (OP_OVERFLOW); hist[op code]: ops the evaluator runs (the dead steps behind an OP_SKIP are
# not counted, the OP_SKIP itself is)
ChunkProgram = namedtuple("ChunkProgram", "chunk prog_len hist on_list")


class Census:
    def __init__(self, chunks, counters, n_nodes):
        self.chunks = chunks      # [ChunkProgram], every listed chunk once
        self.counters = counters  # (class 0, class 1, class 2, long entries of class 0, short entries of class 0)
        self.n_nodes = n_nodes    # processed nodes of the program that was stepped (None: not given)

    @property
    def lists(self):
        return self.counters[:3]

    @property
    def overflow_chunks(self):
        """chunks evaluated on the full program"""
        return sum(1 for c in self.chunks if c.prog_len is None)

    @property
    def overflow_is_poisoned(self):
        """Every node emits at most one op, so a program of at most OP_CAP processed nodes cannot overflow by length: its OP_OVERFLOW chunks
        are `poisoned` ones (a saturation-class drop followed by a combination behind the 14-position test). True / False where that can
        be told, None for a longer program (either cause) or an unknown node count."""
        if self.n_nodes is None or self.n_nodes > OP_CAP:
            return None
        return self.overflow_chunks > 0

    @property
    def poisoned_chunks(self):
        return self.overflow_chunks if self.overflow_is_poisoned else 0

    def hist(self):
        """[compact programs, 8] op-code histograms of the chunks that have a compact program (the shape `live_programs` returned)"""
        return np.array([c.hist for c in self.chunks if c.prog_len is not None]).reshape(-1, 8)

    def op_total(self, op):
        return int(sum(c.hist[op] for c in self.chunks if c.prog_len is not None))

    def max_prog_len(self, on_list=None):
        lens = [c.prog_len for c in self.chunks if c.prog_len is not None and (on_list is None or c.on_list in on_list)]
        return max(lens) if lens else 0

    def on(self, *lists):
        return [c for c in self.chunks if c.on_list in lists]


def census(obj, n_nodes=None, rolled=True):
    """Census of `obj`'s last sample stage. `rolled`: the step ran the derive sweep behind the sampler, which rolls the list counters over
    into their statistics words (role_preset); False after a step of the sample stage alone, whose counters are still live."""
    lib = capi.lib()
    lib.ivx_grid_device_ptr.restype = C.c_void_p
    hip = C.CDLL("libamdhip64.so")
    n = obj.n_chunks
    lens = np.zeros(4 * n + 16, dtype=np.uint32)
    ops = np.zeros((n, OP_CAP, 2), dtype=np.uint32)
    hip.hipDeviceSynchronize()
    assert hip.hipMemcpy(lens.ctypes.data_as(C.c_void_p), C.c_void_p(lib.ivx_grid_device_ptr(obj.h, 7)), lens.nbytes, 2) == 0
    assert hip.hipMemcpy(ops.ctypes.data_as(C.c_void_p), C.c_void_p(lib.ivx_grid_device_ptr(obj.h, 8)), ops.nbytes, 2) == 0
    base = n + (8 if rolled else 0)
    cnt = tuple(int(v) for v in lens[base:base + 5])  # [0..3) the three lists, [3] long and [4] short entries of the first
    assert cnt[0] == cnt[3] + cnt[4], cnt
    chunks = []
    for c in range(3):
        seg = lens[n + 16 + c * n:n + 16 + (c + 1) * n]
        if c == 0:
            entries = [(int(ch), LISTS[0]) for ch in seg[:cnt[3]]] + [(int(ch), LISTS[1]) for ch in seg[n - cnt[4]:]]
        else:
            entries = [(int(ch), LISTS[c + 1]) for ch in seg[:cnt[c]]]
        for ch, name in entries:
            ln = int(lens[ch])
            h = np.zeros(8, dtype=np.int64)
            if ln == OP_OVERFLOW:
                chunks.append(ChunkProgram(ch, None, h, name))
                continue
            assert ln <= OP_CAP, (ch, ln)
            i = 0
            while i < ln:
                o = int(ops[ch, i, 0] >> 28)
                h[o] += 1
                if o == OP_SKIP:  # (a dropped first operand's steps: the evaluator jumps over them)
                    assert int(ops[ch, i, 1]) >= 1, (ch, i)
                    i += int(ops[ch, i, 1])
                else:
                    i += 1
            chunks.append(ChunkProgram(ch, ln, h, name))
    assert len({c.chunk for c in chunks}) == len(chunks) == sum(cnt[:3]), (len(chunks), cnt)
    return Census(chunks, cnt, n_nodes)
