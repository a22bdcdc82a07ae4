"""Device cells of a chain group (ceg_mc_group_set_device_cells), the parts that need no device: ceg_hip.mcrng.CellBook -- the NumPy
restatement of the cell lists whose sequential semantics the accept launch replays -- against hand-computed cases, its bin_of on
lattice faces, the bindings against the header, and the new symbols in the built library."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from ceg_hip import _abi, mcrng

HEADER = Path(__file__).resolve().parent.parent / "include" / "ceg_hip.h"
NEW = ("ceg_mc_group_set_device_cells", "ceg_mc_group_halted", "ceg_mc_cell_lists")


def _book(cells):
    """a 10 A cubic MC cell cut into 2 x 2 x 2 bins (cell = 4 bx + 2 by + bz); `cells`: per atom slot the cell it starts in"""
    book = mcrng.CellBook(np.eye(3) / 10.0, (2, 2, 2))
    centre = {c: np.array([2.5 + 5.0 * (c >> 2), 2.5 + 5.0 * ((c >> 1) & 1), 2.5 + 5.0 * (c & 1)]) for c in range(8)}
    book.set_atoms(np.array([centre[c] for c in cells]))
    return book, centre


def _consistent(book):
    for c, mem in enumerate(book.members):
        for i, slot in enumerate(mem):
            assert (book.cell_of[slot], book.idx_of[slot]) == (c, i)
    assert sum(len(m) for m in book.members) == len(book.cell_of) == len(book.idx_of)


def test_take_out_of_the_last_and_of_a_middle_entry():
    book, _ = _book([0, 0, 0, 0])
    assert book.members[0] == [0, 1, 2, 3] and book.max_fill == 4
    book.take_out(3)                                             # the last entry: nothing moves
    assert book.members[0] == [0, 1, 2] and 3 not in book.cell_of
    book.take_out(0)                                             # a middle entry: the last one moves into the hole
    assert book.members[0] == [2, 1] and book.idx_of[2] == 0 and book.idx_of[1] == 1
    book.put_in(3, 0)
    assert book.members[0] == [2, 1, 3] and book.idx_of[3] == 2
    book.take_out(7)                                             # a slot in no cell: nothing
    assert book.members[0] == [2, 1, 3] and book.max_fill == 4
    _consistent(book)


def test_two_atoms_of_one_molecule_leave_the_same_cell():
    """cell 0 = [0 1 2 3 4], the molecule in slots 1, 2 moves to cell 7: atom 1 out -> [0 4 2 3], atom 2 (entry 2) out -> [0 4 3]"""
    book, centre = _book([0, 0, 0, 0, 0])
    assert book.move(1, [centre[7], centre[7]]) == 2
    assert book.members[0] == [0, 4, 3] and book.members[7] == [1, 2]
    assert [book.idx_of[s] for s in (0, 4, 3, 1, 2)] == [0, 1, 2, 0, 1]
    _consistent(book)
    assert book.move(1, [centre[7] + 0.5, centre[7] - 0.5]) == 0         # same bins: refreshed in place
    assert book.members[7] == [1, 2]


def test_an_atom_enters_the_cell_another_atom_of_the_molecule_just_left():
    """cell 0 = [0 2], cell 1 = [1 3]; the molecule in slots 0, 1 swaps its two cells.  Atom 0: out of cell 0 -> [2], into cell 1 ->
    [1 3 0]; atom 1 (entry 0 of cell 1): the last entry, atom 0, moves into the hole -> [0 3], then into cell 0 -> [2 1]"""
    book, centre = _book([0, 1, 0, 1])
    assert book.members[0] == [0, 2] and book.members[1] == [1, 3]
    assert book.move(0, [centre[1], centre[0]]) == 2
    assert book.members[0] == [2, 1] and book.members[1] == [0, 3]
    assert (book.cell_of[0], book.idx_of[0]) == (1, 0) and (book.cell_of[1], book.idx_of[1]) == (0, 1)
    assert book.max_fill == 3                                    # cell 1 held three entries for a moment: the capacity it needs
    _consistent(book)


def test_deletion_with_renumbering_of_the_last_molecule():
    """cell 0 = [0 1 2 3 4 5]: the molecule in slots 0-2 goes, the last molecule (slots 3-5) takes its index.  Out 0 -> [5 1 2 3 4],
    out 1 -> [5 4 2 3], out 2 -> [5 4 3]; the refresh of slots 3-5 changes no list"""
    book, centre = _book([0] * 6)
    book.remove(0, 3, 3, 3)
    assert book.members[0] == [5, 4, 3] and [book.idx_of[s] for s in (5, 4, 3)] == [0, 1, 2]
    assert all(s not in book.cell_of for s in (0, 1, 2))
    book.insert(0, [centre[0], centre[3], centre[0]])            # the freed slots are used again
    assert book.members[0] == [5, 4, 3, 0, 2] and book.members[3] == [1]
    cell_of, idx_of = book.lists(7)
    assert cell_of.tolist() == [0, 3, 0, 0, 0, 0, -1] and idx_of.tolist() == [3, 0, 4, 2, 1, 0, -1]
    assert cell_of.dtype == np.int32 and idx_of.dtype == np.int32
    _consistent(book)


def test_bin_of_on_lattice_faces():
    book = mcrng.CellBook(np.eye(3), (4, 3, 2))                  # positions are fractional coordinates
    cell = lambda b: (b[0] * 3 + b[1]) * 2 + b[2]
    assert book.bin_of([0.0, 0.0, 0.0]) == 0
    assert book.bin_of([0.25, 1.0 / 3.0, 0.5]) == cell((1, 1, 1))                    # on a face: the upper bin
    assert book.bin_of([np.nextafter(0.25, 0.0), 0.0, np.nextafter(0.5, 0.0)]) == cell((0, 0, 0))
    assert book.bin_of([1.0, 2.0, -3.0]) == 0                                       # whole cells away: f - floor(f) = 0
    assert book.bin_of([np.nextafter(1.0, 0.0)] * 3) == cell((3, 2, 1))
    # f = 1 - 1e-17 is 1.0 in FP64 and wraps to bin 0; f = -1e-17 gives f - floor(f) = 1.0: truncated to nb, clamped to nb - 1
    assert 1.0 - 1e-17 == 1.0 and book.bin_of([1.0 - 1e-17] * 3) == 0
    assert book.bin_of([-1e-17] * 3) == cell((3, 2, 1))
    assert book.bin_of([5.75, -0.5, 0.49]) == cell((3, 1, 0))
    # a triclinic cell: the fractional coordinates come from invmat @ p
    mat = np.array([[10.0, 2.0, 1.0], [0.0, 9.0, 3.0], [0.0, 0.0, 8.0]])
    tri = mcrng.CellBook(np.linalg.inv(mat), (5, 5, 5))
    for f in ([0.1, 0.5, 0.9], [0.39, 0.61, 0.01], [0.99, 0.21, 0.79]):
        b = [int(x * 5) for x in f]
        assert tri.bin_of(mat @ np.array(f)) == (b[0] * 5 + b[1]) * 5 + b[2], f


def test_replay_of_a_sweep_log():
    """replay_cell_book on a hand-written log: accepted moves only, idle (-1) and stopped (-2) records change nothing"""
    book, centre = _book([0, 1, 0, 1])
    log = np.zeros(4, dtype=_abi.SWEEP_RECORD_DTYPE)
    log["molecule"] = [0, 0, -2, -1]
    log["accepted"] = [0, 1, 1, 1]
    log["positions"][:, 0], log["positions"][:, 1] = centre[1], centre[0]
    changed = mcrng.replay_cell_book(book, log, first_slot=[0, 2], atoms=[2, 2])
    assert changed == 2 and book.members[0] == [2, 1] and book.members[1] == [0, 3]


def test_prototypes_match_the_header():
    text = HEADER.read_text()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"CEG_API int (ceg_mc_\w+)\(([^;]*?)\);", text, re.S)}
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int32_t*": _abi.c_int32_p, "int64_t*": _abi.c_int64_p,
             "ceg_mc_group_t*": C.c_void_p, "ceg_mc_t*": C.c_void_p}
    for name in NEW:
        assert name in decl, name
        args = [re.sub(r"/\*.*?\*/", "", a, flags=re.S).strip() for a in decl[name].split(",")]
        types = [re.sub(r"\s*\w+$", "", a).replace(" *", "*") for a in args]
        restype, argtypes = _abi.PROTOTYPES[name]
        assert restype is C.c_int and argtypes == [ctype[t] for t in types], (name, types)


def test_the_built_library_exports_the_new_entry_points():
    lib = C.CDLL(str(Path(_abi.LIB_PATH)))
    for name in NEW:
        assert hasattr(lib, name), name
