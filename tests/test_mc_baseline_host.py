"""ceg_mc_baseline / ceg_mc_group_baseline at the boundary, without a GPU: the two symbols are exported and bound, the record of
`ceg_hip/_abi.py` has the size and the field offsets of `ceg_mc_baseline_t` in include/ceg_hip.h (measured by a C compiler on the
header itself), and the argument checks refuse before anything touches a device."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

from ceg_hip import _abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ceg_hip.h"
FIELDS = ("framework_vdw", "framework_direct", "inter", "recip_framework", "recip_guests", "nmol", "natoms")


def test_both_symbols_are_exported_and_bound():
    lib = _abi.load_library()
    for name in ("ceg_mc_baseline", "ceg_mc_group_baseline"):
        assert name in _abi.PROTOTYPES
        fn = getattr(lib, name)                         # AttributeError if the library does not export it
        assert fn.restype is C.c_int and len(fn.argtypes) == 3
    text = HEADER.read_text()
    m = re.search(r"#define\s+CEG_MC_BASELINE_REFRESH\s+(\d+)", text)
    assert m and int(m.group(1)) == _abi.MC_BASELINE_REFRESH == 1


def test_record_layout_is_the_headers(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "a C compiler is needed to measure ceg_mc_baseline_t"
    src = tmp_path / "layout.c"
    prints = "\n".join(f'    printf("{f} %zu\\n", offsetof(ceg_mc_baseline_t, {f}));' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ceg_hip.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(ceg_mc_baseline_t));\n' + prints + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    dt = _abi.MC_BASELINE_DTYPE
    assert int(got["sizeof"]) == dt.itemsize == 48
    assert dt.names == FIELDS
    for f in FIELDS:
        assert int(got[f]) == dt.fields[f][1], (f, got[f], dt.fields[f][1])
    assert all(dt.fields[f][0] == "<f8" for f in FIELDS[:5]) and all(dt.fields[f][0] == "<i4" for f in FIELDS[5:])


def test_bad_arguments_are_refused_before_any_launch():
    """NULL handle / group, NULL out, unknown flag bits -> CEG_ERR_INVALID with a message.  The stand-in for a handle is a zeroed
    buffer: these checks come before the handle is looked at, so it is never read."""
    lib = _abi.load_library()
    rec = (C.c_char * 48)()
    fake = (C.c_char * 4096)()
    handle, out = C.addressof(fake), C.addressof(rec)
    for fn in (lib.ceg_mc_baseline, lib.ceg_mc_group_baseline):
        for args, word in (((None, 0, out), b"NULL"), ((handle, 0, None), b"NULL"), ((None, 0, None), b"NULL"),
                           ((handle, 2, out), b"flag"), ((handle, _abi.MC_BASELINE_REFRESH | 4, out), b"flag"), ((handle, -1, out), b"flag")):
            assert fn(*args) == -1, (fn.__name__, args)
            assert word in lib.ceg_last_error(), (fn.__name__, args, lib.ceg_last_error())
    assert bytes(rec) == bytes(48) and bytes(fake) == bytes(4096)
