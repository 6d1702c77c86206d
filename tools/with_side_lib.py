"""Run one of the tools on another build of a side library: the module's SIDE.path is set before the tool imports or uses it.
   usage: python tools/with_side_lib.py NAME=PATH [NAME=PATH ...] tools/TOOL.py [the tool's arguments]
   e.g.   python tools/with_side_lib.py elevation=build/parent/libpgtt_elevation.so tools/gpu_elevation_time.py --fill 4 --out profiles/NAME.txt
NAME is render, depth, perceive, elevation, learn or lidar.  This is how a timing tool is run on the parent commit's library and on the new one
in the same job, alternating; the tool's build_info lines then say which source each run was built from."""
import importlib
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    args = sys.argv[1:]
    while args and "=" in args[0] and not args[0].endswith(".py"):
        name, path = args.pop(0).split("=", 1)
        mod = importlib.import_module("phase_guided_terrain_traversal_amd." + name)
        mod.SIDE.path = os.path.abspath(path)
    if not args:
        sys.exit(__doc__)
    sys.argv = args
    runpy.run_path(args[0], run_name="__main__")


if __name__ == "__main__":
    main()
