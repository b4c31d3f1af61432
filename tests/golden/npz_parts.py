"""Golden arrays stored as several small archives: ``<stem>.00.npz``, ``<stem>.01.npz``, ...

One ``np.savez_compressed`` archive per part, each kept below PART_LIMIT bytes so that no
committed fixture grows past 1 MiB.  ``save_parts`` fills the parts greedily in the order of
``arrays``; ``load_parts`` gives the arrays back by name, whichever part holds them.
"""
import glob
import os
import zlib

import numpy as np

PART_LIMIT = 900 * 1024
_MEMBER_OVERHEAD = 512          # zip headers + the .npy header, per array (an upper estimate)


def part_paths(directory, stem):
    return sorted(glob.glob(os.path.join(directory, glob.escape(stem) + ".[0-9][0-9].npz")))


def save_parts(directory, stem, arrays):
    """Write ``arrays`` (name -> ndarray) as ``<stem>.NN.npz`` parts; returns their paths."""
    for old in part_paths(directory, stem):
        os.remove(old)
    parts, cur, size = [], {}, 0
    for name, a in arrays.items():
        a = np.asarray(a)
        cost = len(zlib.compress(np.ascontiguousarray(a).tobytes(), 6)) + _MEMBER_OVERHEAD
        if cost > PART_LIMIT:
            raise ValueError(f"{name}: {cost} compressed bytes do not fit one part")
        if cur and size + cost > PART_LIMIT:
            parts.append(cur)
            cur, size = {}, 0
        cur[name] = a
        size += cost
    if cur:
        parts.append(cur)
    paths = []
    for i, part in enumerate(parts):
        path = os.path.join(directory, f"{stem}.{i:02d}.npz")
        np.savez_compressed(path, **part)
        paths.append(path)
    return paths


class PartedArrays:
    """Read-only mapping over the parts of one stem (the interface tests use of np.load)."""

    def __init__(self, directory, stem):
        paths = part_paths(directory, stem)
        if not paths:
            raise FileNotFoundError(f"no {stem}.NN.npz under {directory}")
        self._files = [np.load(p) for p in paths]
        self._where = {}
        for f in self._files:
            for name in f.files:
                if name in self._where:
                    raise ValueError(f"{name} is stored in two parts of {stem}")
                self._where[name] = f
        self.files = list(self._where)

    def __getitem__(self, name):
        return self._where[name][name]

    def __contains__(self, name):
        return name in self._where

    def __iter__(self):
        return iter(self.files)

    def __len__(self):
        return len(self.files)

    def keys(self):
        return self.files


def load_parts(directory, stem):
    return PartedArrays(directory, stem)
