"""Feature instances: the connected components of a label volume as records.

One :class:`FeatureInstance` per row of the instance table (``ops.ccl.instance_table``): exact
integer counts and bounds, the centroid as ``sum / voxels`` in float64 on the host; with an access
table (``ops.access.access_table``) also the voxels open toward each face of the grid; with a dimension table (``ops.edt.dimension_table``) also its clear width: the
largest squared distance from one of its voxels to the material, and where that voxel lies; with a
reach table (``ops.reach.reach_table``) also what a given tool reaches from each face and clears; with
the contact tables (``ops.contact.contact_table``) also the area of its walls, of its openings and of
the faces it shares with other instances, side by side, and which instances those are; with a wall
table (``ops.nearest.wall_table``) also how close it comes to another instance without touching it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from ..ops.reference import EDT_INF

from .partfeatures import FACES

_AXIS = {"z": 0, "y": 1, "x": 2}


def tool_thresholds(t) -> tuple:
    """``(need2, cut2)`` of a ball-shaped tool of diameter ``t`` voxels (the convention of
    ``FeatureInstance.tool_diameter``), in exact arithmetic: the tool's centre may stand on a voxel
    whose squared distance to the material is at least ``need2 = ceil(((t + 1) / 2)^2)``, and from
    there it removes the voxels within squared distance ``cut2 = floor((t / 2)^2)``.  ``t`` is an
    int, a float (taken at its exact binary value), a ``Fraction`` or a decimal string, ``>= 0``."""
    if isinstance(t, bool):
        raise ValueError(f"tool_thresholds: the tool diameter must be a number, not {t!r}")
    try:
        d = Fraction(t)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"tool_thresholds: the tool diameter must be a finite number, not {t!r}") from None
    if d < 0:
        raise ValueError(f"tool_thresholds: the tool diameter must be >= 0, not {t!r}")
    need2, cut2 = math.ceil(((d + 1) / 2) ** 2), math.floor((d / 2) ** 2)
    if need2 >= EDT_INF:
        raise ValueError(f"tool_thresholds: a tool of diameter {t!r} is wider than any grid")
    return need2, cut2


def wall_threshold(t) -> int:
    """``limit2`` of a wall thickness of ``t`` voxels, in exact arithmetic: a wall of ``w`` whole
    voxels between two features puts their nearest voxel centres ``w + 1`` apart, so the voxels that
    have another feature behind a wall of at most ``t`` voxels are those whose squared distance to it
    is at most ``limit2 = floor((t + 1)^2)``.  ``t`` is an int, a float (taken at its exact binary
    value), a ``Fraction`` or a decimal string, ``>= 0``."""
    if isinstance(t, bool):
        raise ValueError(f"wall_threshold: the wall thickness must be a number, not {t!r}")
    try:
        w = Fraction(t)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"wall_threshold: the wall thickness must be a finite number, not {t!r}") from None
    if w < 0:
        raise ValueError(f"wall_threshold: the wall thickness must be >= 0, not {t!r}")
    limit2 = math.floor((w + 1) ** 2)
    if limit2 >= EDT_INF:
        raise ValueError(f"wall_threshold: a wall of {t!r} voxels is thicker than any grid")
    return limit2


@dataclass
class FeatureInstance:
    """One component of one class in one sample."""
    id: int                  # the component's number in its sample's ``ids`` volume (from 1)
    cls: int                 # its class
    voxels: int
    bbox: tuple              # (z0, y0, x0, z1, y1, x1), bounds inclusive
    centroid: tuple          # (z, y, x), float64
    access: tuple | None = None    # its voxels open toward each face, in FACES order (None: not computed)
    enclosed: int | None = None    # its voxels open toward no face
    clearance2: int | None = None  # the largest squared distance from a voxel's centre to a material voxel's
    clearance_at: tuple | None = None   # (z, y, x) of the first voxel, in raster order, that attains it
    wall_voxels: int | None = None      # its voxels with a material face neighbour
    entry2: tuple | None = None    # per face, the largest squared clearance of a straight path from that face to a voxel
    reachable: tuple | None = None      # per face, its voxels the tool's centre reaches from that face
    unreachable: int | None = None      # its voxels the tool's centre reaches from no face
    machinable: int | None = None       # its voxels the tool removes from the centres it reaches
    tool: tuple | None = None      # (need2, cut2) of the tool these counts were made for
    wall_area: tuple | None = None      # per side, in FACES order, its voxel faces that meet material
    open_area: tuple | None = None      # per side, its voxel faces that meet free space or the outside of the grid
    shared_area: tuple | None = None    # per side, its voxel faces that meet another instance
    neighbors: tuple | None = None      # (id, face, faces): instance ``id`` of the sample lies toward ``face`` on ``faces`` faces
    walls: bool = False            # the four below were computed (they are None where the part has no other instance)
    gap2: int | None = None        # the smallest squared distance from a voxel's centre to another instance's voxel's
    gap_at: tuple | None = None    # (z, y, x) of the first voxel, in raster order, that attains it
    gap_to: int | None = None      # the id, in the sample's ``ids`` volume, of the instance nearest to that voxel
    thin_voxels: int | None = None      # its voxels with another instance within the wall limit (None: no limit given)
    recognized: int | None = None       # the single-feature classifier's class, 0..C-1 (None: not asked, or too small)
    recognized_prob: float | None = None     # its softmax probability
    component: int | None = None   # the id of the connected component a watershed split cut it from (None: no split)
    peak2: int | None = None       # the largest squared distance to the material inside it, as the split saw it
    faces: "np.ndarray | None" = field(default=None, compare=False)    # the triangles of the part's mesh that lie against it, ascending (None: no mesh given)

    @property
    def agrees(self) -> bool | None:
        """The classifier names the class the record carries: ``cls == recognized + 1`` (the label rule
        of ``generate_parts``: label = 1 + class); None where the classifier was not asked."""
        return None if self.recognized is None else self.cls == self.recognized + 1

    @property
    def clearance(self) -> float | None:
        """The distance from the deepest voxel's centre to the nearest material voxel's centre, in
        voxels (``inf`` in a part without material); None without dimensions."""
        if self.clearance2 is None:
            return None
        return math.inf if self.clearance2 >= EDT_INF else math.sqrt(self.clearance2)

    @property
    def tool_diameter(self) -> float | None:
        """The diameter in voxels of the largest ball, centred on a voxel centre, that touches no
        material voxel: ``max(0, 2 * clearance - 1)``; None without dimensions."""
        c = self.clearance
        return None if c is None else max(0.0, 2.0 * c - 1.0)

    @property
    def gap(self) -> float | None:
        """The distance from the centre of the voxel nearest to another instance to the centre of
        that instance's nearest voxel, in voxels; None without walls or alone in the part."""
        return None if self.gap2 is None else math.sqrt(self.gap2)

    @property
    def min_wall(self) -> float | None:
        """The thinnest wall toward another instance, in voxels: ``max(0, gap - 1)`` (0: they share a
        face, edge or corner); None without walls or alone in the part."""
        g = self.gap
        return None if g is None else max(0.0, g - 1.0)

    def entry_diameter(self, face: str) -> float | None:
        """The diameter in voxels of the largest ball that reaches at least one voxel of the feature
        in a straight line from ``face``: ``max(0, 2 * sqrt(entry2) - 1)`` (``inf`` in a part without
        material); None without reach."""
        if face not in FACES:
            raise ValueError(f"entry_diameter: face must be one of {FACES}, not {face!r}")
        if self.entry2 is None:
            return None
        e = self.entry2[FACES.index(face)]
        return math.inf if e >= EDT_INF else max(0.0, 2.0 * math.sqrt(e) - 1.0)

    @property
    def residual(self) -> int | None:
        """The voxels the tool leaves behind: ``voxels - machinable``; None without reach."""
        return None if self.machinable is None else self.voxels - self.machinable

    def tool_faces(self, min_fraction: float = 1.0) -> tuple:
        """The names of the faces from which the tool's centre reaches at least ``min_fraction`` of
        the voxels in a straight line."""
        if self.reachable is None:
            raise ValueError("tool_faces: this instance carries no reach counts (extract_features(tool=...))")
        return tuple(f for f, c in zip(FACES, self.reachable) if c >= min_fraction * self.voxels)

    @property
    def surface(self) -> int | None:
        """The faces of its voxels that are not interior: wall, open and shared, over all sides; None
        without contacts."""
        if self.wall_area is None:
            return None
        return sum(self.wall_area) + sum(self.open_area) + sum(self.shared_area)

    def floor(self, face: str) -> int:
        """The wall area on the side opposite ``face``: what a tool that enters through ``face`` finds
        at the bottom (0 for a hole that goes through)."""
        if face not in FACES:
            raise ValueError(f"floor: face must be one of {FACES}, not {face!r}")
        if self.wall_area is None:
            raise ValueError("floor: this instance carries no contact areas (extract_features(contacts=True))")
        return self.wall_area[FACES.index(face) ^ 1]

    def blind(self, face: str) -> bool:
        """Entered through ``face`` it has a floor: ``floor(face) > 0``."""
        return self.floor(face) > 0

    def entered_through(self, face: str) -> tuple:
        """The ids of the instances of the same sample that lie toward ``face`` of this one."""
        if face not in FACES:
            raise ValueError(f"entered_through: face must be one of {FACES}, not {face!r}")
        if self.neighbors is None:
            raise ValueError("entered_through: this instance carries no contacts (extract_features(contacts=True))")
        return tuple(i for i, f, _ in self.neighbors if f == face)

    def open_faces(self, min_fraction: float = 1.0) -> tuple:
        """The names of the faces toward which at least ``min_fraction`` of the voxels are open:
        no material lies between such a voxel and that face of the grid."""
        if self.access is None:
            raise ValueError("open_faces: this instance carries no access counts (extract_features(access=True))")
        return tuple(f for f, c in zip(FACES, self.access) if c >= min_fraction * self.voxels)

    @property
    def through(self) -> bool:
        """Open toward two opposite faces (a through hole or slot); False without access counts."""
        faces = self.open_faces() if self.access is not None else ()
        return any(FACES[k] in faces and FACES[k + 1] in faces for k in (0, 2, 4))

    def depth(self, face: str) -> int:
        """The extent of the bounding box along the axis of ``face`` (``"+z"`` ... ``"-y"``)."""
        if face not in FACES:
            raise ValueError(f"depth: face must be one of {FACES}, not {face!r}")
        a = _AXIS[face[1]]
        return self.bbox[3 + a] - self.bbox[a] + 1

    def to_dict(self, min_fraction: float = 1.0) -> dict:
        """JSON-safe record; with access counts also ``access`` (face -> voxels), ``open_faces``
        (at ``min_fraction``), ``through`` and ``enclosed``; with dimensions also ``clearance2``,
        ``clearance_at``, ``tool_diameter`` (None where it is unbounded) and ``wall_voxels``; with
        reach also ``tool`` (need2, cut2), ``entry2`` and ``reachable`` (face -> value), ``tool_faces``
        (at ``min_fraction``), ``unreachable``, ``machinable`` and ``residual``; with contacts also
        ``wall_area``, ``open_area``, ``shared_area`` and ``floor`` (face -> faces), ``surface`` and
        ``neighbors`` (a list of ``{"id", "face", "faces"}``); with walls also ``gap2``, ``gap_at``,
        ``gap_to``, ``min_wall`` (each None alone in the part) and ``thin_voxels``; with a classifier's
        opinion also ``recognized``, ``recognized_prob`` and ``agrees``; after a watershed split also
        ``component`` and ``peak2``; with a mesh also ``faces``."""
        d = {"id": self.id, "class": self.cls, "voxels": self.voxels, "bbox": list(self.bbox),
             "centroid": list(self.centroid)}
        if self.access is not None:
            d.update(access=dict(zip(FACES, self.access)), open_faces=list(self.open_faces(min_fraction)),
                     through=self.through, enclosed=self.enclosed)
        if self.clearance2 is not None:
            tool = self.tool_diameter
            d.update(clearance2=self.clearance2, clearance_at=list(self.clearance_at),
                     tool_diameter=tool if math.isfinite(tool) else None, wall_voxels=self.wall_voxels)
        if self.reachable is not None:
            d.update(tool=list(self.tool), entry2=dict(zip(FACES, self.entry2)),
                     reachable=dict(zip(FACES, self.reachable)), tool_faces=list(self.tool_faces(min_fraction)),
                     unreachable=self.unreachable, machinable=self.machinable, residual=self.residual)
        if self.wall_area is not None:
            d.update(wall_area=dict(zip(FACES, self.wall_area)), open_area=dict(zip(FACES, self.open_area)),
                     shared_area=dict(zip(FACES, self.shared_area)), floor={f: self.floor(f) for f in FACES},
                     surface=self.surface,
                     neighbors=[{"id": i, "face": f, "faces": c} for i, f, c in self.neighbors])
        if self.walls:
            d.update(gap2=self.gap2, gap_at=None if self.gap_at is None else list(self.gap_at), gap_to=self.gap_to,
                     min_wall=self.min_wall, thin_voxels=self.thin_voxels)
        if self.recognized is not None:
            d.update(recognized=self.recognized, recognized_prob=self.recognized_prob, agrees=self.agrees)
        if self.component is not None:
            d.update(component=self.component, peak2=self.peak2)
        if self.faces is not None:
            d.update(faces=[int(i) for i in self.faces])
        return d

    @staticmethod
    def from_table(table, offsets, min_voxels: int = 1, access=None, dims=None, shape=None, reach=None,
                   tool=None, contacts=None, walls=None, thin: bool = True,
                   recognized=None, split=None) -> "list[list[FeatureInstance]]":
        """Per-sample record lists from an instance table int64 ``[T, 13]`` and its ``offsets``
        ``[N + 1]`` (tensors or arrays).  Components of fewer than ``min_voxels`` voxels are left
        out; the others keep their ``id``.  ``access``: the access table int64 ``[T, 8]`` of the
        same rows, or None.  ``dims``: the dimension table int64 ``[T, 4]`` of the same rows, or None;
        with it ``shape``, the ``(D, H, W)`` of a sample, which turns ``at`` into ``(z, y, x)``.
        ``reach``: the reach table int64 ``[T, 15]`` of the same rows, or None; with it ``tool``, the
        ``(need2, cut2)`` it was made for.  ``contacts``: ``(contact, adj)``, the contact table int64
        ``[T, 19]`` of the same rows and its pair list int64 ``[P, 4]``, or None; a neighbour that
        ``min_voxels`` leaves out of the lists still appears in ``neighbors``, by its id.  ``walls``:
        the wall table int64 ``[T, 5]`` of the same rows, or None; it needs ``shape`` too, and with
        ``thin=False`` (no limit was asked for) ``thin_voxels`` stays None.  ``recognized``: ``(cls,
        prob)`` of ``ops.isolate.recognize_table``, int64 and float32 ``[T]`` of the same rows, or None;
        a row with ``cls < 0`` was not classified and keeps None.  ``split``: ``(parent_component, peak2)``
        of ``ops.watershed.split_instances``, int64 ``[T]`` of the same rows, or None."""
        tab = np.asarray(table.cpu() if hasattr(table, "cpu") else table, dtype=np.int64).reshape(-1, 13)
        off = np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets, dtype=np.int64)
        acc = None
        if access is not None:
            acc = np.asarray(access.cpu() if hasattr(access, "cpu") else access, dtype=np.int64).reshape(-1, 8)
            if len(acc) != len(tab) or not np.array_equal(acc[:, 7], tab[:, 2]):
                raise ValueError("from_table: the access table does not belong to this instance table")
        dim = None
        if dims is not None:
            dim = np.asarray(dims.cpu() if hasattr(dims, "cpu") else dims, dtype=np.int64).reshape(-1, 4)
            if len(dim) != len(tab) or not np.array_equal(dim[:, 3], tab[:, 2]):
                raise ValueError("from_table: the dimension table does not belong to this instance table")
            if shape is None or len(shape) != 3:
                raise ValueError("from_table: dims needs shape = (D, H, W)")
            _, H, W = (int(s) for s in shape)
        rch = None
        if reach is not None:
            rch = np.asarray(reach.cpu() if hasattr(reach, "cpu") else reach, dtype=np.int64).reshape(-1, 15)
            if len(rch) != len(tab) or not np.array_equal(rch[:, 14], tab[:, 2]):
                raise ValueError("from_table: the reach table does not belong to this instance table")
            if tool is None or len(tool) != 2:
                raise ValueError("from_table: reach needs tool = (need2, cut2)")
            tool = (int(tool[0]), int(tool[1]))
        con = near = None
        if contacts is not None:
            con, adj = (np.asarray(t.cpu() if hasattr(t, "cpu") else t, dtype=np.int64) for t in contacts)
            con, adj = con.reshape(-1, 19), adj.reshape(-1, 4)
            if len(con) != len(tab) or not np.array_equal(con[:, 18], tab[:, 2]):
                raise ValueError("from_table: the contact table does not belong to this instance table")
            if len(adj) and (adj[:, :2].min() < 0 or adj[:, :2].max() >= len(tab) or adj[:, 2].min() < 0
                             or adj[:, 2].max() > 5):
                raise ValueError("from_table: the contact pairs do not belong to this instance table")
            first = off[np.searchsorted(off, np.arange(len(tab)), side="right") - 1]    # the first row of each row's sample
            near = [[] for _ in range(len(tab))]
            for a, b, k, faces in adj.tolist():      # a sees b toward k, b sees a toward the opposite side
                near[a].append((b - int(first[b]) + 1, k, faces))
                near[b].append((a - int(first[a]) + 1, k ^ 1, faces))
        wal = None
        if walls is not None:
            wal = np.asarray(walls.cpu() if hasattr(walls, "cpu") else walls, dtype=np.int64).reshape(-1, 5)
            if len(wal) != len(tab) or not np.array_equal(wal[:, 4], tab[:, 2]):
                raise ValueError("from_table: the wall table does not belong to this instance table")
            if shape is None or len(shape) != 3:
                raise ValueError("from_table: walls needs shape = (D, H, W)")
            _, H, W = (int(s) for s in shape)
        rec_cls = rec_prob = None
        if recognized is not None:
            rec_cls, rec_prob = (np.asarray(t.cpu() if hasattr(t, "cpu") else t).reshape(-1) for t in recognized)
            if len(rec_cls) != len(tab) or len(rec_prob) != len(tab):
                raise ValueError("from_table: the recognized classes do not belong to this instance table")
        comp = None
        if split is not None:
            comp, peak = (np.asarray(t.cpu() if hasattr(t, "cpu") else t, dtype=np.int64).reshape(-1) for t in split)
            if len(comp) != len(tab) or len(peak) != len(tab):
                raise ValueError("from_table: the split columns do not belong to this instance table")
        out = []
        for n in range(len(off) - 1):
            recs = []
            for k in range(int(off[n]), int(off[n + 1])):
                row = tab[k]
                vox = int(row[2])
                if vox < min_voxels:
                    continue
                cen = row[10:13].astype(np.float64) / np.float64(vox)
                rec = FeatureInstance(id=k - int(off[n]) + 1, cls=int(row[1]), voxels=vox,
                                      bbox=tuple(int(v) for v in row[4:10]),
                                      centroid=tuple(float(c) for c in cen))
                if acc is not None:
                    rec.access, rec.enclosed = tuple(int(c) for c in acc[k, :6]), int(acc[k, 6])
                if dim is not None:
                    r2, at, wall = (int(v) for v in dim[k, :3])
                    rec.clearance2, rec.wall_voxels = r2, wall
                    rec.clearance_at = (at // (H * W), at // W % H, at % W)
                if rch is not None:
                    rec.entry2, rec.reachable = tuple(int(v) for v in rch[k, :6]), tuple(int(v) for v in rch[k, 6:12])
                    rec.unreachable, rec.machinable, rec.tool = int(rch[k, 12]), int(rch[k, 13]), tool
                if con is not None:
                    rec.wall_area, rec.open_area = tuple(int(v) for v in con[k, :6]), tuple(int(v) for v in con[k, 6:12])
                    rec.shared_area = tuple(int(v) for v in con[k, 12:18])
                    rec.neighbors = tuple((i, FACES[f], c) for i, f, c in sorted(near[k]))
                if wal is not None:
                    gap2, at, other = (int(v) for v in wal[k, :3])
                    rec.walls, rec.thin_voxels = True, int(wal[k, 3]) if thin else None
                    if gap2 >= 0:
                        rec.gap2, rec.gap_at = gap2, (at // (H * W), at // W % H, at % W)
                        rec.gap_to = other - int(off[n]) + 1
                if rec_cls is not None and rec_cls[k] >= 0:
                    rec.recognized, rec.recognized_prob = int(rec_cls[k]), float(rec_prob[k])
                if comp is not None:
                    rec.component, rec.peak2 = int(comp[k]), int(peak[k])
                recs.append(rec)
            out.append(recs)
        return out


def assign_faces(features, winners) -> None:
    """Fill ``FeatureInstance.faces`` of every record: ``features`` is one list of records per
    sample and ``winners`` one int32 ``[F_i]`` array per sample (``label_mesh``'s: the id that lies
    against each triangle of the sample's mesh, 0 for none).  A record gets the indices of the
    triangles its id won, ascending; ids without a record keep their triangles to themselves."""
    for recs, win in zip(features, winners):
        win = np.asarray(win)
        order = np.argsort(win, kind="stable")
        start = np.concatenate([[0], np.cumsum(np.bincount(win, minlength=1))])
        for rec in recs:
            rec.faces = order[start[rec.id]:start[rec.id + 1]] if rec.id + 1 < len(start) else order[:0]
