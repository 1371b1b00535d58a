"""The one loader of the scalar reference libraries (tests/*_ref/): make, load, set prototypes, once per process.

The first call for a directory always runs its Makefile, whether or not the .so is there: make is incremental, and a stale library once
hid a checker change. Later calls return the cached handle and fork nothing."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}


def load(ref_dir, lib_file, symbols):
    """The library tests/<ref_dir>/<lib_file>, brought up to date with its sources, with `symbols` (name -> (restype, argtypes)) applied."""
    key = (ref_dir, lib_file)
    if key not in _libs:
        path = os.path.join(HERE, ref_dir)
        subprocess.run(["make", "-s", "-C", path], check=True)
        lib = C.CDLL(os.path.join(path, lib_file))
        for name, (res, args) in symbols.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _libs[key] = lib
    return _libs[key]
