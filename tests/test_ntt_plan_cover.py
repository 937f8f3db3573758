"""The shape table of the transform-driver tests (tests/ntt_driver_shapes.py) covers every class of launch the drivers can make for
k <= 20, logb <= 4, every shard_log and batches on both sides of the 64 MiB footprint threshold (up to 128 MiB) - classes as sp_ntt_plan,
the code that launches the passes, reports them.  No GPU: the plan is host arithmetic.  A change to geometry() or the tile rules that
moves a test shape off its path fails here and names the class that lost its test."""
import numpy as np

import ntt_driver_shapes as shapes
from ntt_driver_shapes import Shape
from lambdaworks_cairo_prover_amd import _lib, api


def _missing(envelope, have):
    """classes of the envelope outside `have`, each with the smallest shape that launches it"""
    out = {}
    for s in sorted(set(envelope), key=lambda s: (shapes.footprint(s), s)):
        for c in shapes.pass_classes(s):
            if c not in have and c not in out:
                out[c] = s
    return out


def test_plan_fields_follow_the_rules_of_the_launcher(hip_lib):
    """sp_ntt_plan against the numbers the drivers are documented to use (csrc/ntt.h), and its argument checks"""
    fwd = api.ntt_plan("forward_natural", 22)
    assert [(p["s"], p["r"], p["g"]) for p in fwd] == [(0, 8, 2), (8, 8, 2), (16, 6, 4)]          # 14 = 8 + 6, not 7 + 7
    assert [(p["load"], p["contig"], p["gtw"], p["weak_out"], p["stage_tw"]) for p in fwd] == [(1, 1, 0, 1, 1), (0, 0, 1, 1, 1), (0, 0, 1, 0, 1)]
    inv = api.ntt_plan("inverse_natural", 22)
    assert [(p["s"], p["r"], p["g"]) for p in inv] == [(16, 6, 4), (8, 8, 2), (0, 8, 2)] and all(p["dif"] for p in inv)
    assert [p["store"] for p in inv] == [0, 0, 1]
    for plan in (fwd, inv):
        for p in plan:
            assert p["tiles"] << (p["r"] + p["g"]) == 1 << p["log_len"] and p["xcd_map"] == int(p["tiles"] % 8 == 0)
            assert p["radix4"] == int(p["r"] >= 2 and p["r"] + p["g"] == 10)
    # the coset-major LDE: contiguous first pass with the transform's table, one launch for all cosets of all columns; 1024-element
    # strided tiles only above 64 MiB
    small, large = api.ntt_plan("lde_coset_major", 12, 3, 0, 3), api.ntt_plan("lde_coset_major", 12, 3, 0, 65)
    assert [(p["contig"], p["gtw"], p["vectors"], p["coset_count"], p["stage_tw"]) for p in small] == [(1, 1, 24, 8, 0), (0, 1, 24, 8, 0)]
    assert (small[1]["r"] + small[1]["g"], small[1]["radix4"]) == (9, 0) and (large[1]["r"] + large[1]["g"], large[1]["radix4"]) == (10, 1)
    # the natural LDE on one coset per rank: expand pass at local stride 0, one element per row
    one = api.ntt_plan("lde_natural", 9, 2, 2, 1)
    assert (one[0]["load"], one[0]["contig"], one[0]["s"], one[0]["g"], one[0]["log_len"]) == (2, 0, 0, 0, 9)
    assert api.ntt_plan("dit_bitrev_to_natural", 0) == [] and len(api.ntt_plan("intt_bitrev", 0)) == 1
    assert api.ntt_plan("lde_natural", 12, 0, 0, 2) == api.ntt_plan("dit_bitrev_to_natural", 12, 0, 0, 2)
    import ctypes
    count = ctypes.c_uint32()
    bad = [(9, 5, 0, 0, 1), (0, 31, 0, 0, 1), (4, 20, 11, 0, 1), (4, 5, 2, 3, 1), (0, 5, 1, 0, 1), (0, 5, 0, 0, 0), (5, 20, 4, 0, 1 << 20)]
    for driver, k, logb, shard_log, batch in bad:
        assert hip_lib.sp_ntt_plan(driver, k, logb, shard_log, batch, None, 0, ctypes.byref(count)) == _lib.SP_E_INVALID_ARG, (driver, k, logb, shard_log, batch)
    assert hip_lib.sp_ntt_plan(0, 5, 0, 0, 1, None, 0, None) == _lib.SP_E_INVALID_ARG
    one_pass = (_lib.NttPassC * 1)()
    assert hip_lib.sp_ntt_plan(0, 22, 0, 0, 1, one_pass, 1, ctypes.byref(count)) == _lib.SP_E_INVALID_ARG and count.value == 3


def test_reference_codec_is_the_products(hip_lib):
    """tests/ntt_driver_ref.py's device layout (Python integers) and the library's host codec agree, so the GPU tests may encode
    their expected values with either"""
    import ntt_driver_ref as ref
    raw = np.random.default_rng(3).integers(0, 256, size=(500, 32), dtype=np.uint8)
    raw[:, 0] &= 0x07
    for i, v in enumerate((api.P - 1, api.P - 2, 0, 1)):
        raw[i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    assert np.array_equal(ref.to_device(raw), api.fe_to_device(raw))
    assert np.array_equal(ref.from_device(api.fe_to_device(raw)), raw)


def test_driver_table_covers_every_class_of_the_envelope(hip_lib):
    envelope = list(shapes.envelope(shapes.DRIVER_TABLE_DRIVERS))
    assert len(envelope) > 2000
    missing = _missing(envelope, shapes.classes_of(shapes.table()))
    assert not missing, "no test shape launches: " + "; ".join(f"[{shapes.describe(c)}] (e.g. {tuple(s)})" for c, s in list(missing.items())[:5])
    # the required shapes are all there, whatever the cover needs
    table = set(shapes.table())
    left_out = []
    for k in (0, 1, 5, 8, 10, 11, 13, 16, 17, 18):
        for logb in (1, 2, 3):
            for batch in (1, 3):
                if Shape("lde_coset_major", k, logb, 0, batch) not in table:
                    left_out.append((k, logb, batch))
    assert left_out == [(17, 3, 3), (18, 2, 3), (18, 3, 3)] or left_out == [(18, 2, 3), (18, 3, 3)]      # 96 MiB and more; (17, 3, 3) is required below
    assert Shape("lde_coset_major", 12, 3, 0, 65) in table and Shape("lde_coset_major", 17, 3, 0, 3) in table
    assert shapes.footprint(Shape("lde_coset_major", 12, 3, 0, 65)) > shapes.FOOTPRINT_THRESHOLD >= shapes.footprint(Shape("lde_coset_major", 12, 3, 0, 64))
    for k in (0, 3, 9, 12, 17):
        for logb in (1, 2):
            for shard_log in range(logb + 1):
                assert Shape("lde_natural", k, logb, shard_log, 1) in table
    for k in (0, 1, 2, 7, 10, 11, 15, 16, 18):
        assert Shape("intt_bitrev", k, 0, 0, 1) in table and Shape("intt_bitrev", k, 0, 0, 5) in table


def test_driver_table_is_the_greedy_cover(hip_lib):
    """COVER is what the required shapes leave uncovered, smallest footprint first, and no row of it is idle: each launches a class
    that neither the required shapes nor the rows before it launch"""
    rows, _ = shapes.greedy_cover(shapes.envelope(shapes.DRIVER_TABLE_DRIVERS), shapes.classes_of(shapes.REQUIRED))
    assert rows == shapes.COVER, (sorted(set(rows) - set(shapes.COVER))[:5], sorted(set(shapes.COVER) - set(rows))[:5])
    assert len(set(shapes.table())) == len(shapes.table())


def test_existing_transform_tests_plus_the_extra_cases_cover_sp_ntt_dev(hip_lib):
    """forward_natural and inverse_natural are reached through sp_ntt and sp_ntt_dev: the (k, batch) lists of the existing tests, read
    from the test functions, together with NTT_DEV_EXTRA cover the envelope"""
    cases = shapes.existing_ntt_cases()
    assert {(0, 1), (13, 5), (19, 3), (22, 1)} <= set(cases) and len(cases) >= 20
    envelope = list(shapes.envelope(shapes.NTT_DRIVERS))
    have = shapes.classes_of(shapes.existing_ntt_shapes())
    rows, _ = shapes.greedy_cover(envelope, have)
    assert rows == shapes.NTT_DEV_EXTRA, rows
    assert rows and all(shapes.footprint(s) > shapes.FOOTPRINT_THRESHOLD for s in rows)       # what the lists miss: small k above 64 MiB
    missing = _missing(envelope, have | shapes.classes_of(shapes.NTT_DEV_EXTRA))
    assert not missing, "; ".join(shapes.describe(c) for c in missing)
