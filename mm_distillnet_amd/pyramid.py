"""Row layout of a feature pyramid held in ONE row buffer (the last BiFPN cell's outputs and every tensor of the heads).

Host arithmetic only (csrc/common.h mmd_make_pyr restated): no kernel library, no tensor library - t[a:b] works on anything sliceable.
"""
import ctypes
from typing import Dict, List, Sequence, Tuple


class Pyramid:
    """B images at `sizes` = [(H, W)] per level: level l holds rows[l] = B*H*W rows from row0[l], every level starting on a 128-row tile."""

    def __init__(self, B: int, sizes: Sequence[Tuple[int, int]]):
        self.B, self.sizes = B, [tuple(s) for s in sizes]
        self.rows: List[int] = [B * h * w for h, w in self.sizes]
        self.row0: List[int] = [0]
        for r in self.rows:
            self.row0.append(self.row0[-1] + (r + 127) // 128 * 128)
        self.total = self.row0[-1]
        self.padded = self.total != sum(self.rows)      # some level ends inside a tile: the buffer has padding rows
        self._descs: Dict[int, ctypes.Array] = {}
        self.desc = self.head_desc(len(self.sizes))     # what the mmd_*_pyr entry points take: {levels, B, H0, W0, H1, W1, ...}

    def head_desc(self, nsplit: int):
        """The descriptor of the leading `nsplit` levels only (built once); all levels: `desc` itself."""
        d = self._descs.get(nsplit)
        if d is None:
            flat = [nsplit, self.B] + [v for hw in self.sizes[:nsplit] for v in hw]
            d = self._descs[nsplit] = (ctypes.c_int * len(flat))(*flat)
        return d

    def level(self, t, l: int):
        """level l's rows of a pyramid row buffer"""
        return t[self.row0[l]:self.row0[l] + self.rows[l]]

    def levels(self, t) -> list:
        return [self.level(t, l) for l in range(len(self.rows))]
