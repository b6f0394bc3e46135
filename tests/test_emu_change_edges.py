"""change() on the CPU emulation at the edges of its wave-wide list walks (tests/change_probe.py: the probe harness and the case tables; families A - F of
DESIGN.md §1 a13), in every lane order the emulation offers and with the element list in LDS and in "global" scratch.  Every made Change is compared with the
oracle's, Change for Change, and the spans of every grown replica with the oracle applying log + wanted Changes.  The emulation builds its ballots lane by lane
and opens its gaps with a plain loop: tests/test_gpu_change_edges.py runs the same tables through the device's own primitives."""
import os

import pytest

import change_probe as CP
import helpers as H

pytestmark = [pytest.mark.skipif(not os.path.exists(H.EMU_LIB), reason="tests/emu/libperitext_emu.so not built (run __graft_entry__.build())"),
              pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]

FORMS = [(0, False), (1, False), (2, False), (0, True), (2, True)]  # (lane order, list in scratch: family F)


class EmuBackend:
    def __init__(self, reverse=0, list_in_hbm=False):
        self.reverse, self.list_in_hbm = reverse, list_in_hbm

    def change_and_grow(self, batch, ops):
        res = H.emu_merge(batch, reverse=self.reverse, admission=True)
        lds = CP.lds_bytes_without_lists(batch, ops) if self.list_in_hbm else H.LDS_BYTES
        made, status = H.emu_change(batch, res, ops, lds_bytes=lds, reverse=self.reverse)
        grown = H.concat_batches(batch, made)
        return made, status, grown, H.emu_merge(grown, reverse=self.reverse, admission=True)


@pytest.mark.parametrize("reverse,list_in_hbm", FORMS)
@pytest.mark.parametrize("family", sorted(CP.FAMILIES))
def test_single_replica_families(family, reverse, list_in_hbm):
    """A: select across chunks (+ out-of-bounds logs beside good ones), B: lookAfterTombstones across chunks, C: the gap opener, D: this call's own elements"""
    CP.run_cases(EmuBackend(reverse, list_in_hbm), CP.FAMILIES[family]())


def test_family_A_positions_come_from_the_base_log():
    """the indices of family A hit list positions 63, 64, 65, 127, 128 and the last visible element: the oracle's text of the base is the builder's"""
    for phase, b, targets in CP.bases_A():
        assert sorted(targets) == ([63, 64, 127, 299] if phase == 2 else [64, 65, 127, 128, 299])
        assert H.oracle_apply([[b.log]])[0][0]["text"] == b.text()
        assert all(b.vis_pos[b.index_of(p)] == p for p in targets)


@pytest.mark.parametrize("reverse,list_in_hbm", FORMS)
def test_generated_replicas_every_replica_edits(reverse, list_in_hbm):
    docs, calls, actors = CP.family_E_generated()
    want = CP.run(EmuBackend(reverse, list_in_hbm), docs, calls, actors, expect_status=[0] * len(actors))
    assert all(w["error"] is None and len(w["changes"]) == 10 for w in want)  # no case dropped
    assert any(len(c["deps"]) == 3 for w in want for c in w["changes"])        # the deps name the other actors


@pytest.mark.parametrize("reverse,list_in_hbm", FORMS)
def test_mixed_sizes_in_one_batch(reverse, list_in_hbm):
    docs, calls, actors = CP.family_E_mixed()
    CP.run(EmuBackend(reverse, list_in_hbm), docs, calls, actors, expect_status=[0, 0, 0, 0])
