"""The large-batch cases of tests/large_batches.py satisfy what they are derived for, checked without a device: (a) the named
array exceeds its mark, (b) the mark lies strictly inside a frame, (c) two whole frames lie beyond it, (d) the call's peak stays
under the cap -- and every family of the inventory has a case or is recorded as per-frame."""
import pytest

from tests import large_batches as L

CASES = L.cases()


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_crosses_its_mark_inside_a_frame(case):
    bpf, n, mark = case.target_bpf, case.n, case.mark
    assert mark in (L.MARK31, L.MARK32, L.MARK34)
    assert case.W % 2 == 1 and case.H % 2 == 1                  # odd sides: no frame size divides a power of two
    assert bpf * n > mark                                        # (a)
    assert mark % bpf != 0                                       # (b) not on a frame boundary
    k = mark // bpf                                              # the frame that holds the mark
    assert k * bpf < mark < (k + 1) * bpf
    assert n - (k + 1) >= 2                                      # (c)
    assert n - (k + 1) == 2                                      # and no larger than that asks for
    if case.target != "C" and case.arrays and case.target in {a.name for a in case.arrays}:
        unit = {a.name: a.unit for a in case.arrays}[case.target]
        assert bpf % unit == 0
    # every other array of the case above 2^31 bytes is crossed inside a frame too
    for a in case.arrays:
        for m in (L.MARK31, L.MARK32, L.MARK34):
            if a.bytes_per_frame * n > m:
                assert m % a.bytes_per_frame != 0, f"{a.name}: a frame boundary falls on {m}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_peak_stays_under_the_cap(case):
    assert L.peak(case) < L.CAP, f"{case.id}: {L.peak(case) / L.GIB:.1f} GiB"            # (d)
    # the reference runs in sub-batches in which every array, and the caller's tensors, stay below 2^31 bytes
    assert 1 <= case.sub_batch < case.n
    for a in case.arrays:
        assert a.bytes_per_frame * case.sub_batch < L.MARK31
    assert case.target_bpf * case.sub_batch < L.MARK31
    # 32-bit pixel indices of the outputs hold for the whole batch
    assert case.n * case.W * case.H < L.MARK31


def test_fused_cases_state_which_arrays_cross_what():
    """Family 1: besides dC the volumes of the pipeline cross 2^32 bytes (and, being bytes, 2^31 elements); the hand-off, state,
    checkpoint and record arrays are listed with what they reach at that batch."""
    for case in (c for c in CASES if c.family == "epi_plan/fused"):
        crossed = {name: (over32, idx31) for name, _, over32, idx31 in L.crossings(case)}
        assert crossed["dC"] == (True, True)
        by_name = {a.name: a.bytes_per_frame * case.n for a in case.arrays}
        if "band" in case.pipeline:
            assert crossed["dX"] == (True, True)
            assert by_name["dBandEdge"] < L.MARK31               # the hand-off maps stay small: W * states * lpp uint4 a frame
            if case.paths == 8:
                assert L.MARK31 // 4 < by_name["dBits"] < L.MARK31   # the bit plane: below 2^31 bytes, above 2^29
        else:
            assert crossed["dLh"] == (True, True)
            assert by_name["dCkpt"] < L.MARK31
        assert by_name["dRec"] < L.MARK31 and by_name["dS0"] < L.MARK31


def test_lines_case_keeps_C_below_the_mark():
    (case,) = [c for c in CASES if c.id == "lines-p8-L"]
    by_name = {a.name: a.bytes_per_frame * case.n for a in case.arrays}
    assert by_name["dL"] > L.MARK32 and by_name["dC"] < L.MARK31


def test_sgm_over_2_34_does_not_fit_the_cap():
    """Why the 2^34 case stops after the ingest: the whole of torch_ops.sgm there holds more than the cap in its cheapest pipeline"""
    assert L.sgm_over_2_34_peak() > L.CAP
    (case,) = [c for c in CASES if c.family == "ingest_hwd"]
    assert case.target_bpf * case.n > L.MARK34 and L.peak(case) < L.CAP


def test_stereo_sgm_pp_across_4_gib_does_not_fit_the_cap():
    """Why family stereo_pp runs the chain's kernels on the caller's maps and not the whole of stereo_sgm_pp"""
    assert L.stereo_sgm_pp_peak() > L.CAP


def test_every_family_has_a_case_or_a_record():
    with_case = {c.family for c in CASES}
    for family, (kind, why) in L.FAMILIES.items():
        assert kind in ("arrays", "per-frame") and why
        if kind == "arrays":
            assert family in with_case, f"{family} has batch-sized arrays and no case"
        else:
            assert family not in with_case
    assert with_case <= set(L.FAMILIES)


def test_helpers_restate_the_host_code():
    """Spot values of the *_bytes helpers at the KITTI shape, worked out by hand from epi_sweep.hip / epi_band.hip"""
    W, H, D = 1242, 375, 128
    assert L.packed_lpp(D) == 8 and L.packed_lpp(300) == 0 and L.packed_lpp(48) == 0
    assert L.band_rows(D) == 64
    assert L.pair_ckpt_bytes(W, H, D, 0) == 375 * 155 * 128      # ceil(1242 / 8) = 156 tiles
    assert L.pair_ckpt_bytes(W, H, D, 1) == 1242 * 46 * 128      # ceil(375 / 8) = 47
    names = [a.name for a in L.epi_plan_arrays(W, H, D, 8, "band16chain/nowrap")]
    assert "dBits" in names and "dL" not in names
    edge = {a.name: a for a in L.epi_plan_arrays(W, H, D, 8, "band16chain/nowrap")}["dBandEdge"]
    assert edge.bytes_per_frame == 5 * 1242 * 3 * 8 * 16         # 6 bands: 5 boundaries
