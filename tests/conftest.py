import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-opencl-raytracer_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through librtamd.so on the GPU)")


def golden_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and not f.endswith(".ref.npz"))


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


_REFERENCE_DATA = []


def reference_data():
    """The folder of the reference's own scene files that the loader tests are pinned to, laid out
    as its data/ folder: collada/cubes2.DAE, models/cubes2.obj, sphere.obj.  They are stored
    xz-compressed under tests/golden/reference_data and unpacked once per session into a
    temporary folder, removed at exit."""
    if not _REFERENCE_DATA:
        import atexit
        import lzma
        import shutil
        import tempfile
        src = os.path.join(GOLDEN, "reference_data")
        dst = tempfile.mkdtemp(prefix="rtamd_reference_data_")
        atexit.register(shutil.rmtree, dst, ignore_errors=True)
        for sub, _, files in os.walk(src):
            out = os.path.join(dst, os.path.relpath(sub, src))
            os.makedirs(out, exist_ok=True)
            for f in files:
                if f.endswith(".xz"):
                    with lzma.open(os.path.join(sub, f)) as fi, open(os.path.join(out, f[:-3]), "wb") as fo:
                        shutil.copyfileobj(fi, fo)
        _REFERENCE_DATA.append(dst)
    return _REFERENCE_DATA[0]


@pytest.fixture(scope="session")
def renderer():
    import rtamd
    r = rtamd.Renderer(0)
    yield r
    r.close()
