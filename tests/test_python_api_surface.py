"""The Python face of the library keeps the surface it had before it was cut into modules, and its handle base closes once.

python_api_surface.json, next to this file, is a record of what `import p3d_amd` offered in the commit BEFORE the split
(the one-file package): every non-dunder, non-module name with its kind; the repr of constants and tables; fields and size
of every ctypes.Structure; the signature of every function and of every public method (and whether it is a property or a
generator function); after lib(), restype and argtypes of every entry point that has a prototype; EXPORTS, sorted.  The tree
under test must offer all of it unchanged; names that are new are free.

The record is made once, from the parent commit and not from the tree under test, with the collector of this module:

    git archive <parent> | tar -x -C /some/scratch/parent          # a checkout of the parent, outside the tree
    P3D_LIB=$PWD/p3d-raytracer_amd/libp3d.so \\
        python tests/test_python_api_surface.py /some/scratch/parent tests/python_api_surface.json

(P3D_LIB: any built libp3d.so of the same ABI, so that the checkout need not be built; LIB_PATH is recorded by kind only for
that reason, and the checkout's own path is written as <ROOT>.)  Regenerate it only when a change of the surface is the
point of a commit, from that commit's parent plus the intended change."""
import ctypes
import inspect
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "python_api_surface.json")
PLAIN = (type(None), bool, int, float, str, bytes, tuple, list, dict)


def _type_name(t):
    return "None" if t is None else t.__name__


def _signature(f):
    try:
        return str(inspect.signature(f))
    except (TypeError, ValueError):
        return "no signature"


def _callable(f):
    return {"signature": _signature(f), "generator": inspect.isgeneratorfunction(f)}


def _own(cls):
    """the public attributes a class defines itself or takes from a base of the package (not from object, tuple or ctypes)"""
    bases = [b for b in cls.__mro__ if b.__module__ not in ("builtins", "_ctypes", "ctypes")]
    return sorted({k for b in bases for k in vars(b) if not k.startswith("_")})


def _class(cls):
    out = {"init": _signature(cls), "members": {}}
    if issubclass(cls, ctypes.Structure):
        out["fields"] = [[f[0], _type_name(f[1])] for f in cls._fields_]
        out["sizeof"] = ctypes.sizeof(cls)
    for k in _own(cls):
        v = inspect.getattr_static(cls, k)
        if isinstance(v, property):
            out["members"][k] = {"kind": "property"}
        elif inspect.isfunction(v):
            out["members"][k] = dict(_callable(v), kind="method")
        else:
            out["members"][k] = {"kind": type(v).__name__}
    return out


def collect(root):
    """The surface of the p3d_amd of the tree at `root`, as plain data.  Imports it: call this in a process of its own, or
    for the tree the process has imported already."""
    if root not in sys.path:
        sys.path.insert(0, root)
    import p3d_amd as p3d
    assert os.path.dirname(os.path.abspath(p3d.__file__)) == os.path.abspath(root), p3d.__file__
    names = {}
    for k, v in sorted(vars(p3d).items()):
        if k.startswith("__") or isinstance(v, types.ModuleType):
            continue
        if inspect.isclass(v):
            names[k] = dict(_class(v), kind="structure" if issubclass(v, ctypes.Structure) else "class")
        elif inspect.isfunction(v):
            names[k] = dict(_callable(v), kind="function")
        elif isinstance(v, PLAIN) and k != "LIB_PATH":
            names[k] = {"kind": type(v).__name__, "repr": repr(v).replace(os.path.abspath(root), "<ROOT>")}
        else:
            names[k] = {"kind": type(v).__name__}
    L = p3d.lib()
    entries = set(p3d.EXPORTS) | set(getattr(p3d, "PROTOTYPES", ())) | {k for k in vars(L) if k.startswith("p3d_")}
    prototypes = {}
    for k in sorted(entries):
        f = getattr(L, k)
        prototypes[k] = {"restype": _type_name(f.restype),
                         "argtypes": "not set" if f.argtypes is None else [_type_name(t) for t in f.argtypes]}
    return {"names": names, "prototypes": prototypes, "exports": sorted(p3d.EXPORTS)}


def test_the_package_offers_what_the_one_file_package_offered():
    record = json.load(open(RECORD))
    now = json.loads(json.dumps(collect(ROOT)))  # (tuples become lists, as in the record)
    assert now["exports"] == record["exports"]
    for part in ("names", "prototypes"):
        gone = sorted(set(record[part]) - set(now[part]))
        assert not gone, "%s that are gone: %s" % (part, gone)
        changed = {k: (v, now[part][k]) for k, v in record[part].items() if now[part][k] != v}
        assert not changed, "%s that changed (before, now): %r" % (part, changed)


def test_importing_the_package_does_not_import_torch():
    code = "import sys; sys.path.insert(0, %r); import p3d_amd; sys.exit(1 if 'torch' in sys.modules else 0)" % ROOT
    assert subprocess.run([sys.executable, "-c", code], timeout=60).returncode == 0


class _Stub:
    """what stands in for the library: one destroy entry point that counts, and fails when told to"""

    def __init__(self):
        self.destroyed, self.fail = [], False

    def stub_destroy(self, h):
        self.destroyed.append(h)
        if self.fail:
            raise RuntimeError("destroy failed")


def _stub_class():
    import p3d_amd as p3d

    class Thing(p3d._Handle):
        _destroy = "stub_destroy"

        def __init__(self, L, fail_early=False):
            self._L = L
            if fail_early:
                raise ValueError("refused before the handle exists")
            self._h = 7

    return Thing


def test_handle_base_destroys_once_and_tolerates_half_made_objects():
    Thing = _stub_class()
    L = _Stub()
    t = Thing(L)
    t.close()
    t.close()
    assert L.destroyed == [7] and t._h is None
    t.__del__()  # after close(): nothing more
    assert L.destroyed == [7]
    half = Thing.__new__(Thing)  # the constructor raised before _h (here: before anything) was set
    half.close()
    half.__del__()
    try:
        Thing(L, fail_early=True)
    except ValueError:
        pass
    assert L.destroyed == [7]


def test_handle_base_del_swallows_what_destroy_raises():
    Thing = _stub_class()
    L = _Stub()
    L.fail = True
    t = Thing(L)
    t.__del__()
    assert L.destroyed == [7]
    try:
        Thing(L).close()  # close() itself does not hide it
    except RuntimeError:
        pass
    else:
        raise AssertionError("close() swallowed the destroy function's exception")


if __name__ == "__main__":
    json.dump(collect(os.path.abspath(sys.argv[1])), open(sys.argv[2], "w"), indent=1, sort_keys=True)
    print("wrote", sys.argv[2])
