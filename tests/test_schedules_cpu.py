"""Every emulator-backed unit under the adversarial fiber schedules of tests/emu/emu.cpp (emu.SCHEDULES: descending, lone-wave, two
seeded random orders).  The default schedule runs lane 0 .. 63 and wave 0 first, so "lane i + 1 reads what lane i wrote" and "wave 1
reads what wave 0 wrote" always see the new value: a missing wave_sync() or block_barrier() can hide behind it.  Here the fiber
tests of the units' own CPU files run again, unchanged -- their sets, their check helpers, their yardsticks (the oracle, the plain
restatements, the host library) -- with the unit's runner bound to a schedule through its `schedule=` argument.  Nothing is
compared with the ascending run of the code under test.

Orders that are unspecified by design (what an atomic that returns the old value hands out: deferral lists, tickets) may differ
between schedules, on the emulator as on the card; outputs may not.  The units' tests compare outputs, and where they look at
tier_footprint's `deferred` they look at one entry or at membership; test_the_deferral_list_is_a_multiset below compares a longer
list, as a multiset for that reason.

tests/test_race_probe_cpu.py shows that the schedules see a missing sync; DESIGN section 26 says what they prove and what not."""
import functools
import importlib
import itertools

import pytest

from tests.emu import emu

# what a unit's tests call, and which of its tests run fibers: (module, test function, None or a predicate on its parameters)
CANON = [("tests.emu.emu", "canonicalize_batch"), ("tests.emu.emu", "tier_footprint")]
ONE_ORDER = "as_built"                  # length_sets.ORDERS: the second order holds the same records behind one filler record
# Thinned, so that the four schedules cost no more than four ascending runs of the same sets (DESIGN section 26 has the times); every
# length class and every boundary stays, repeats of a class go:
#   length_sets: one of the two orders of every route, and of the mixed sweeps' three output sets the one with bytes and hash;
#   monomerize: not test_adversarial_seed_1, two thirds of the unit's time: the adversarial records a fourth time (seeds 5, 10 and
#     63 run), and a seed of 1 runs on every length in test_every_length.  monomerize.h has no LDS access and no sync.
UNITS = {
    "canonicalize": (CANON, [
        ("tests.test_emu_kernel", "test_staged_streaming_geometries", None),                   # every geometry of STAGED_GEOMETRIES
        ("tests.test_emu_kernel", "test_deferral_to_bigger_tier", None),
        ("tests.test_emu_kernel", "test_team_mode_four_waves_one_record", None),
        ("tests.test_emu_kernel", "test_team_mode_with_n_bitmask", None),
        ("tests.test_emu_kernel", "test_team_mode_four_bit", None),
        ("tests.test_emu_kernel", "test_mixed_kernel_lean_routines", None),                    # the mixed-length pure and N builds
        ("tests.test_emu_kernel", "test_mixed_kernel_prefix_rule_and_extension_edges", None),
        ("tests.test_emu_kernel", "test_mixed_kernel_settles_a_tied_minimal_key", None),
        ("tests.test_emu_kernel", "test_mixed_kernel_winner_seen_twice_by_one_lane", None),
        ("tests.test_emu_kernel", "test_mixed_kernel_minimal_key_inside_a_reverse_complement_palindrome", None),
        ("tests.test_emu_kernel", "test_mixed_kernel_n_inside_the_minimal_window_is_resolved_among_the_sharers", None),
        ("tests.test_emu_kernel", "test_mixed_kernel_with_fused_xxh3", None),
        ("tests.test_emu_kernel", "test_pair_build_two_records_per_wave", None),
        ("tests.test_emu_kernel", "test_streaming_n_build_fuses_the_hash_of_records_with_n", None),
        ("tests.test_length_sets_cpu", "test_streaming_sweeps_take_the_intended_routine", lambda p: p["order"] == ONE_ORDER),
        ("tests.test_length_sets_cpu", "test_mixed_sweeps_take_the_lean_routines", lambda p: p["order"] == ONE_ORDER and p["outs"] == "bh"),
        ("tests.test_tier_sets_cpu", "test_stage_boundary_on_the_emulator", None),             # one wave, the team pass, wave 0 alone
        ("tests.test_tier_sets_cpu", "test_tight_predicates_reach_their_last_dword", None),
        ("tests.test_tier_sets_cpu", "test_mixed_kernel_boundary_on_the_emulator", None),
    ]),
    "scan": ([("tests.emu.scan_emu", "run")], [
        ("tests.test_scan_cpu", "test_block_scan", None),
        ("tests.test_scan_cpu", "test_second_level_rounds", None),
        ("tests.test_scan_cpu", "test_tile_base", None),
        ("tests.test_scan_cpu", "test_composed_scan", None),
        ("tests.test_scan_cpu", "test_composed_scan_wide_tiles", None),
        ("tests.test_scan_cpu", "test_saturation_inside_a_tile", None),
        ("tests.test_scan_cpu", "test_saturation_between_rounds", None),
        ("tests.test_scan_cpu", "test_state_operand_order", None),
    ]),
    "fasta_parse": ([("tests.emu.fasta_emu", "run")], [
        ("tests.test_fasta_device_cpu", "test_small_texts", None),
        ("tests.test_fasta_device_cpu", "test_large_texts", None),
        ("tests.test_fasta_device_cpu", "test_tile_edges", None),
        ("tests.test_fasta_device_cpu", "test_capacities_and_refusals", None),
    ]),
    "fasta_write": ([("tests.emu.fasta_write_emu", "run")], [
        ("tests.test_fasta_write_cpu", "test_device_routines_as_fibers", None),
        ("tests.test_fasta_write_cpu", "test_fibers_capacity", None),
        ("tests.test_fasta_write_cpu", "test_fibers_overlap", None),
        ("tests.test_fasta_write_cpu", "test_canonicalize_and_uniq_files", None),
        ("tests.test_fasta_write_cpu", "test_rotate_cat_decat_files", None),
        ("tests.test_fasta_write_cpu", "test_orfs_file", None),
    ]),
    "windows": ([("tests.emu.windows_emu", "run")], [
        ("tests.test_windows_cpu", "test_device_routine_as_fibers", None),
        ("tests.test_windows_cpu", "test_fibers_refuse_a_short_capacity", None),
        ("tests.test_windows_cpu", "test_a_payload_across_byte_2_32_as_fibers", None),
    ]),
    "translate": ([("tests.emu.translate_emu", "run")], [
        ("tests.test_translate_cpu", "test_device_routine_as_fibers", None),
        ("tests.test_translate_cpu", "test_fibers_refuse_a_short_capacity", None),
    ]),
    "monomer_compact": ([("tests.emu.compact_emu", "compact")], [
        ("tests.test_monomers_compact_emu", "test_emulator_sets", None),
        ("tests.test_monomers_compact_emu", "test_emulator_sets_shifted", None),
        ("tests.test_monomers_compact_emu", "test_every_misalignment_pair", None),
        ("tests.test_monomers_compact_emu", "test_tile_boundary_on_a_record_boundary_at_every_output_shift", None),
        ("tests.test_monomers_compact_emu", "test_filters_at_their_boundaries", None),
        ("tests.test_monomers_compact_emu", "test_a_payload_across_byte_2_32", None),
    ]),
    "uniq_compact": ([("tests.emu.uniq_compact_emu", "decide")], [
        ("tests.test_uniq_compact_cpu", "test_decide_uniq_on_random_triples", None),
    ]),
    "monomerize": ([("tests.emu.mono_emu", "monomerize_batch")], [
        ("tests.test_monomerize_emu", "test_every_length", None),
        ("tests.test_monomerize_emu", "test_adversarial", None),
        ("tests.test_monomerize_emu", "test_identity_boundaries", None),
        ("tests.test_monomerize_emu", "test_known_answers", None),
        ("tests.test_monomerize_emu", "test_every_alignment_and_position_in_the_batch", None),
    ]),
    "sketch": ([("tests.emu.sketch_emu", "run_sketch"), ("tests.emu.sketch_emu", "run_compare")], [
        ("tests.test_sketch_cpu", "test_known_answers_as_fibers", None),
        ("tests.test_sketch_cpu", "test_every_length_as_fibers", None),                        # length_records at PARAMS, the spans round SEG
        ("tests.test_sketch_cpu", "test_symbols_and_alignments_as_fibers", None),              # symbol_records
        ("tests.test_sketch_cpu", "test_the_hash_that_equals_empty_as_fibers", None),
        ("tests.test_sketch_cpu", "test_compare_as_fibers", None),
    ]),
    "cluster": ([("tests.emu.cluster_emu", "run_candidates"), ("tests.emu.cluster_emu", "run_link")], [
        ("tests.test_cluster_cpu", "test_candidates_as_fibers", None),
        ("tests.test_cluster_cpu", "test_capacity_as_fibers", None),
        ("tests.test_cluster_cpu", "test_one_record_past_the_emit_grid_as_fibers", None),
        ("tests.test_cluster_cpu", "test_link_as_fibers", None),                               # link_cases and contention(small=True)
    ]),
    "prealign": ([("tests.emu.prealign_emu", "run_anchors"), ("tests.emu.prealign_emu", "run_votes"), ("tests.emu.prealign_emu", "run_labels")], [
        ("tests.test_prealign_cpu", "test_anchors_as_fibers", None),                           # anchor_cases: the sketch unit's anchors sweep
        ("tests.test_prealign_cpu", "test_votes_as_fibers", None),
        ("tests.test_prealign_cpu", "test_labels_as_fibers", None),
    ]),
    "distance": ([("tests.emu.distance_emu", "run")], [
        ("tests.test_distance_cpu", "test_the_sets_as_fibers", None),                          # all of distance_sets.cases()
    ]),
    "prims": ([("tests.emu.prims_emu", "run")], [
        ("tests.test_prims_cpu", "test_emulator_keeps_the_contract", None),
    ]),
}


def _parameters(fn):
    """The parameter sets of a test function, from its parametrize marks: [{name: value}]."""
    axes = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [n.strip() for n in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        rows = [getattr(v, "values", v) for v in mark.args[1]]
        axes.append([dict(zip(names, row if len(names) > 1 else (row,))) for row in rows])
    return [functools.reduce(lambda a, b: {**a, **b}, combo, {}) for combo in itertools.product(*axes)]


def _cells():
    cells = []
    for unit, (_, tests) in UNITS.items():
        for module, name, keep in tests:
            fn = getattr(importlib.import_module(module), name)
            params = [p for p in _parameters(fn) if keep is None or keep(p)]
            assert params, (module, name)
            cells += [pytest.param(unit, module, name, p, id="%s-%s-%d" % (unit, name[5:], k)) for k, p in enumerate(params)]
    return cells


@functools.lru_cache(maxsize=None)
def _fixture(module, name):
    """A module-scoped fixture of the unit's own test file (its cases, its constants, the oracle), made once."""
    f = getattr(importlib.import_module(module), name)
    return (getattr(f, "__wrapped__", None) or f.__pytest_wrapped__.obj)()


@pytest.mark.parametrize("schedule", emu.SCHEDULES)
@pytest.mark.parametrize("unit,module,name,params", _cells())
def test_unit_under_schedule(unit, module, name, params, schedule, tmp_path, monkeypatch):
    calls = []
    for runner_module, attr in UNITS[unit][0]:
        m = importlib.import_module(runner_module)
        plain = getattr(m, attr)

        def bound(*a, _plain=plain, **kw):
            calls.append(1)
            return _plain(*a, schedule=schedule, **kw)
        monkeypatch.setattr(m, attr, bound)
    fn = getattr(importlib.import_module(module), name)
    wanted = fn.__code__.co_varnames[:fn.__code__.co_argcount]
    kw = {a: params[a] if a in params else tmp_path if a == "tmp_path" else _fixture(module, a) for a in wanted}
    fn(**kw)
    assert calls, "the test ran no fibers through the unit's runner: the schedule was not applied"


@pytest.mark.parametrize("schedule", ("ascending",) + emu.SCHEDULES)
def test_the_deferral_list_is_a_multiset(schedule):
    """Eleven records too long for stage A's workgroup, dealt to its four waves among empty ones: every one is passed on unwritten.
    The order of the list is the order in which the waves' atomic adds on the deferral counter came, which is the schedule's; what
    is in it is not.  Compared as a multiset with what the list must hold, which follows from the lengths alone."""
    from tests import seqsets
    from tests import tier_sets as T
    last = [t for t in T.TRIPLES if t.stage == "A" and t.cls == "pure" and not t.nxt.startswith("stage A")]
    beyond = max(T.triple_n_max(t) for t in last) + 1           # one more than the last route of stage A admits
    long = [k for k in range(16) if k % 3 != 1]
    seqs = [T.make("pure", beyond + k, 11 + k) if k in long else b"" for k in range(16)]
    data, offs = seqsets.pack(seqs)
    r = emu.tier_footprint(data, offs, T.STAGE_SLICE["A"], "tier", entries=list(range(16)), schedule=schedule)
    assert r["status"] == 0 and r["guard_touched"] == 0
    assert sorted(e & 0x3FFFFFFF for e in r["deferred"]) == long
    assert (r["bytes"] == emu.S_OUT).all() and all(r["index"][k] == emu.S_IDX for k in long)
