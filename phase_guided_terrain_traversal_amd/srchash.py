"""SHA-256 over what physics_kernel is built from (stdlib only: csrc/Makefile runs this file to embed the hash in libpgtt.so, native.py imports
it): the include closure of the translation unit csrc/pgtt_physics_inst.hip - itself, the two physics headers, the common header, include/pgtt.h -
and csrc/flags.mk, the make fragment that holds the compile flags of that unit.  Comments and white space are removed (a comment edit does not
change the kernel).  The task-side kernels, the host code and the other rules of the Makefile are not covered: a change there leaves the hash,
and with it the counters recorded under profiles/, valid.  EXTRA flags and the 1-ulp division are what the build's flavor says.

The side libraries (csrc/pgtt_side.mk) embed a hash of their own, side_sha256("render" | "depth" | "perceive" | "elevation" | "learn" | "lidar"): the
include closure of their one translation unit, normalised the same way.  SIDE_SOURCES is the one statement of what a side library is built from:
the hash, the make file's prerequisites and the closure test of tests/test_abi.py read it.  `python3 srchash.py` prints the physics hash,
`python3 srchash.py render` a side hash, `python3 srchash.py --files render` the files that hash covers, one per line."""
import hashlib
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
PHYSICS_SOURCES = ("pgtt_physics_inst.hip", "pgtt_physics.hip.h", "pgtt_physics_quad.hip.h", "pgtt_common.hip.h")
FLAGS_FRAGMENT = "flags.mk"
# per side library: the unit and the shared headers in csrc/, then the public headers in include/ (every project file the unit includes)
_PRELUDE = ("pgtt_side_host.h",)
_DEVICE = ("pgtt_side_device.hip.h",)                       # Philox: the four libraries whose kernels draw
_RAYCAST = ("pgtt_raycast.hip.h", "pgtt_raycast_host.h") + _PRELUDE
_SENSOR = ("pgtt_sensor.hip.h",) + _DEVICE + _RAYCAST       # the two onboard ray sensors
SIDE_SOURCES = {"render": (("pgtt_render.hip",) + _RAYCAST, ("pgtt_render.h", "pgtt.h")),
                "depth": (("pgtt_depth.hip",) + _SENSOR, ("pgtt_depth.h", "pgtt_render.h", "pgtt.h")),
                "perceive": (("pgtt_perceive.hip",) + _PRELUDE, ("pgtt_perceive.h", "pgtt.h")),
                "elevation": (("pgtt_elevation.hip",) + _DEVICE + _PRELUDE, ("pgtt_elevation.h", "pgtt.h")),
                "learn": (("pgtt_learn.hip",) + _DEVICE + _PRELUDE, ("pgtt_learn.h", "pgtt.h")),
                "lidar": (("pgtt_lidar.hip",) + _SENSOR, ("pgtt_lidar.h", "pgtt_render.h", "pgtt.h"))}


def hashed_files(pkg: str = _HERE):
    """the files the hash covers, for the package directory `pkg` (the checkout's by default)"""
    return sorted([os.path.join(pkg, "csrc", f) for f in PHYSICS_SOURCES + (FLAGS_FRAGMENT,)] + [os.path.join(os.path.dirname(pkg), "include", "pgtt.h")])


def side_files(name: str, pkg: str = _HERE):
    """the files side_sha256(name) covers"""
    csrc, include = SIDE_SOURCES[name]
    return sorted([os.path.join(pkg, "csrc", f) for f in csrc] + [os.path.join(os.path.dirname(pkg), "include", f) for f in include])


def source_sha256(pkg: str = _HERE) -> str:
    return _sha256(hashed_files(pkg))


def side_sha256(name: str, pkg: str = _HERE) -> str:
    return _sha256(side_files(name, pkg))


def _sha256(files) -> str:
    h = hashlib.sha256()
    for f in files:
        with open(f, "r") as fh:
            text = fh.read()
        if f.endswith(".mk"):
            text = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
        else:
            text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
            text = re.sub(r"//[^\n]*", " ", text)
        h.update(os.path.basename(f).encode() + b"\0" + " ".join(text.split()).encode() + b"\0")
    return h.hexdigest()


if __name__ == "__main__":
    import sys
    args = sys.argv[1:]
    if args[:1] == ["--files"]:
        print("\n".join(side_files(args[1])))
    else:
        print(side_sha256(args[0]) if args else source_sha256())
