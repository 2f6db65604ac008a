"""The stored fixtures under ``tests/golden/reference`` as a directory of plain files.

The two large text fixtures (``nas_5_5_10.xml``, ``datasets/10Products.pdt``) are stored
xz-compressed; :func:`ref_dir` unpacks the tree once per process into a temporary directory
(removed at exit) and returns its path.
"""
import atexit
import functools
import lzma
import os
import shutil
import tempfile

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")


@functools.lru_cache(maxsize=None)
def ref_dir() -> str:
    dst = tempfile.mkdtemp(prefix="fn_golden_")
    atexit.register(shutil.rmtree, dst, ignore_errors=True)
    for root, _, files in os.walk(SRC):
        out = os.path.join(dst, os.path.relpath(root, SRC))
        os.makedirs(out, exist_ok=True)
        for f in files:
            if f.endswith(".xz"):
                with lzma.open(os.path.join(root, f)) as fi, open(os.path.join(out, f[:-3]), "wb") as fo:
                    shutil.copyfileobj(fi, fo)
            else:
                shutil.copy(os.path.join(root, f), os.path.join(out, f))
    return dst
