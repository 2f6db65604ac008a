"""Feature instances: the connected components of a label volume as records.

One :class:`FeatureInstance` per row of the instance table (``ops.ccl.instance_table``): exact
integer counts and bounds, the centroid as ``sum / voxels`` in float64 on the host.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class FeatureInstance:
    """One component of one class in one sample."""
    id: int                  # the component's number in its sample's ``ids`` volume (from 1)
    cls: int                 # its class
    voxels: int
    bbox: tuple              # (z0, y0, x0, z1, y1, x1), bounds inclusive
    centroid: tuple          # (z, y, x), float64

    def to_dict(self) -> dict:
        """JSON-safe record."""
        return {"id": self.id, "class": self.cls, "voxels": self.voxels, "bbox": list(self.bbox),
                "centroid": list(self.centroid)}

    @staticmethod
    def from_table(table, offsets, min_voxels: int = 1) -> "list[list[FeatureInstance]]":
        """Per-sample record lists from an instance table int64 ``[T, 13]`` and its ``offsets``
        ``[N + 1]`` (tensors or arrays).  Components of fewer than ``min_voxels`` voxels are left
        out; the others keep their ``id``."""
        tab = np.asarray(table.cpu() if hasattr(table, "cpu") else table, dtype=np.int64).reshape(-1, 13)
        off = np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets, dtype=np.int64)
        out = []
        for n in range(len(off) - 1):
            recs = []
            for k in range(int(off[n]), int(off[n + 1])):
                row = tab[k]
                vox = int(row[2])
                if vox < min_voxels:
                    continue
                cen = row[10:13].astype(np.float64) / np.float64(vox)
                recs.append(FeatureInstance(id=k - int(off[n]) + 1, cls=int(row[1]), voxels=vox,
                                            bbox=tuple(int(v) for v in row[4:10]),
                                            centroid=tuple(float(c) for c in cen)))
            out.append(recs)
        return out
