"""Parity of the HIP engine (through the C-ABI) with the CPU restatement and the
reference's golden fixtures.  Bit-exact: texts, visible segments, property
planes, digests, per-doc status and the op statistics must all be equal."""
import numpy as np
import pytest

from fixtures_util import replay_fixtures
from scenarios import PROPS_AT, SCENARIOS, expected_of, props_at, run_scenario
from flat_checks import assert_stopped_like_spec, resident_docs

from fluidframework_amd import gen
from fluidframework_amd.abi import MTE_E_CAPACITY
from fluidframework_amd.engine import DeviceEngine
from oracle import OracleEngine, SpecOracle

pytestmark = pytest.mark.gpu

STAT_KEYS = ["ops_applied", "segs_scanned", "segs_written", "prop_writes", "units_inserted", "max_segs"]


def replay_both(stream, threads=8):
    """The engine and its specification (SpecOracle: the flat restatement for
    new length-calc documents, the tree for legacy ones) on one stream."""
    n_keys = stream["n_keys"]
    o = SpecOracle(n_keys, threads=threads)
    o.load_docs(stream["inits"], stream["init_text"])
    o.apply_batch(stream["batch"])
    d = DeviceEngine(n_keys)
    d.load_docs(stream["inits"], stream["init_text"])
    d.apply_batch(stream["batch"])
    return o, d


def assert_same(o, d, sample_docs=16):
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())
    so, sd = o.stats(), d.stats()
    for k in STAT_KEYS:
        assert sd[k] == so[k], k
    n = o.n_docs
    for doc in sorted(set(np.linspace(0, n - 1, min(n, sample_docs)).astype(int).tolist())):
        assert d.read_doc(doc) == o.read_doc(doc)


def test_gpu_replays_reference_fixtures():
    passed, failures, eng = replay_fixtures(lambda k: DeviceEngine(k))
    assert failures == []
    assert passed == 30 * 64 * 2
    _, _, oeng = replay_fixtures(lambda k: OracleEngine(k), check=False)
    np.testing.assert_array_equal(eng.digest(), oeng.digest())


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_gpu_scenarios(name):
    st_o, text_o, rd_o, _ = run_scenario(SpecOracle(8), name)
    st_d, text_d, rd_d, interner = run_scenario(DeviceEngine(8), name)
    assert st_d == st_o
    for pos, want in PROPS_AT.get(name, []):
        assert props_at(rd_d, interner, pos) == want, pos
    assert rd_d == rd_o
    exp = expected_of(name)
    if exp is not None and not exp.startswith("ERR:"):
        assert text_d == exp


@pytest.mark.parametrize("cfg,n_docs,ops", [(2, 300, 1000), (3, 64, 4000), (4, 2000, 500)])
def test_gpu_matches_oracle_generated(cfg, n_docs, ops):
    s = gen.generate(cfg, n_docs=n_docs, ops_per_doc=ops, doc_base=7)
    o, d = replay_both(s)
    assert (o.statuses() == 0).all()
    assert_same(o, d)


def test_gpu_length_modes_and_keys():
    for mode in (1, 2):
        for n_keys in (0, 4, 8):
            s = gen.generate(3, n_docs=40, ops_per_doc=1500, length_mode=mode)
            if n_keys != 4:
                s["n_keys"] = n_keys
            o, d = replay_both(s)
            assert_same(o, d, sample_docs=4)


def test_gpu_multi_batch_equals_single_batch():
    s = gen.generate(3, n_docs=50, ops_per_doc=3000)
    one = DeviceEngine(s["n_keys"])
    one.load_docs(s["inits"], s["init_text"])
    one.apply_batch(s["batch"])
    many = DeviceEngine(s["n_keys"])
    many.load_docs(s["inits"], s["init_text"])
    b = s["batch"]
    offs = b["op_offsets"].astype(np.int64)
    for lo_frac, hi_frac in [(0, 0.3), (0.3, 0.31), (0.31, 1.0)]:
        parts, new_offs = [], [0]
        for doc in range(50):
            n = offs[doc + 1] - offs[doc]
            lo, hi = offs[doc] + int(n * lo_frac), offs[doc] + int(n * hi_frac)
            parts.append(b["ops"][lo:hi])
            new_offs.append(new_offs[-1] + hi - lo)
        sub = dict(b)
        sub["ops"] = np.concatenate(parts)
        sub["op_offsets"] = np.array(new_offs, np.uint64)
        # text offsets of each batch are relative to that batch's text: resubmit
        # the whole text each time and the engine rebases them
        many.apply_batch(sub)
    np.testing.assert_array_equal(many.digest(), one.digest())


def test_gpu_reset_rerun_is_deterministic():
    s = gen.generate(2, n_docs=100, ops_per_doc=1000)
    d = DeviceEngine(s["n_keys"])
    d.load_docs(s["inits"], s["init_text"])
    d.apply_batch(s["batch"])
    first = d.digest().copy()
    for _ in range(2):
        d.reset()
        d.run()
        d.sync()
        np.testing.assert_array_equal(d.digest(), first)


def test_gpu_large_docs_escalate_register_tiers():
    # insert-only streams grow to hundreds of segments per doc: exercises the
    # E = 1 -> 2 -> 4 -> 8 -> 16 register tiers and the second pass
    s = gen.generate(2, n_docs=24, ops_per_doc=420, mix=gen.MIX_INSERT, min_length=0)
    o, d = replay_both(s)
    assert o.stats()["max_segs"] > 512
    assert_same(o, d, sample_docs=24)


def test_gpu_capacity_error_is_reported():
    s = gen.generate(2, n_docs=4, ops_per_doc=800, mix=gen.MIX_INSERT, min_length=0)
    d = DeviceEngine(s["n_keys"])
    d.load_docs(s["inits"], s["init_text"])
    d.apply_batch(s["batch"])
    o = OracleEngine(s["n_keys"])
    o.load_docs(s["inits"], s["init_text"])
    o.apply_batch(s["batch"])
    assert o.stats()["max_segs"] > 1022
    st = d.statuses()
    assert (st == MTE_E_CAPACITY).all()
    assert_stopped_like_spec(s, d, 1024, streamed=False)  # stops in the last register tier


def replay_both_cap(stream, cap, threads=8):
    n_keys = stream["n_keys"]
    o = SpecOracle(n_keys, threads=threads, cap=cap)
    o.load_docs(stream["inits"], stream["init_text"])
    o.apply_batch(stream["batch"])
    d = DeviceEngine(n_keys, seg_capacity=cap)
    d.load_docs(stream["inits"], stream["init_text"])
    d.apply_batch(stream["batch"])
    return o, d


def test_gpu_chunk_pass_insert_heavy_large_docs():
    # insert-only docs grow past the register tiers (1,022 segments): pass 3,
    # which is chunk_kernel in a context of 8,192 segments and more (launch_replay)
    # (new length calc; legacy documents live in the tree pass, <= 1,020 items)
    s = gen.generate(2, n_docs=12, ops_per_doc=2600, mix=gen.MIX_INSERT, min_length=0, length_mode=2)
    o, d = replay_both_cap(s, 8192)
    assert o.stats()["max_segs"] > 2000
    assert (o.statuses() == 0).all()
    assert_same(o, d, sample_docs=12)


def test_gpu_chunk_pass_long_docs_all_ops():
    # config-5 shaped (scaled down): a long initial text split by insert /
    # remove / annotate ops in deep rounds (1,024 concurrent ops); a 16,384-segment
    # context: the chunked pass (statistics on: op after op)
    s = gen.generate(3, n_docs=6, ops_per_doc=4000, init_len=20000, round_ops=1024, min_length=16,
                     length_mode=2)
    o, d = replay_both_cap(s, 16384)
    assert o.stats()["max_segs"] > 1100
    assert (o.statuses() == 0).all()
    assert_same(o, d, sample_docs=6)


def test_gpu_tree_pass_long_legacy_docs_go_on_in_hbm():
    # the same legacy documents outgrow the register tiers (1,020 items) and go
    # on in the HBM tree pass (mte_htree.h) to the end of the batch, equal to
    # the specification (titems.c) in statuses, digests, statistics and read-outs
    s = gen.generate(3, n_docs=6, ops_per_doc=4000, init_len=20000, round_ops=1024, min_length=16,
                     length_mode=1)
    o, d = replay_both_cap(s, 16384)
    assert (o.statuses() == 0).all()
    assert o.stats()["max_segs"] > 1020
    assert_same(o, d, sample_docs=6)


def test_gpu_tree_pass_capacity_is_the_context_capacity():
    # a legacy document stops with MTE_E_CAPACITY only at the ctx capacity
    s = gen.generate(3, n_docs=4, ops_per_doc=4000, max_lag=32, mix=gen.MIX_INSERT | gen.MIX_ANNOTATE,
                     min_length=16, length_mode=1)
    o, d = replay_both_cap(s, 1536)
    assert (o.statuses() == MTE_E_CAPACITY).all()
    assert o.stats()["max_segs"] > 1020
    assert_same(o, d, sample_docs=4)


def test_gpu_chunk_pass_annotate_heavy():
    # a 16,384-segment context: the chunked pass
    s = gen.generate(3, n_docs=6, ops_per_doc=3000, init_len=6000, round_ops=512, min_length=16,
                     length_mode=2, mix=gen.MIX_INSERT | gen.MIX_ANNOTATE)
    o, d = replay_both_cap(s, 16384)
    assert o.stats()["max_segs"] > 4000
    assert (o.statuses() == 0).all()
    assert_same(o, d, sample_docs=6)


def test_gpu_stream_pass_capacity_error():
    # 1,536 segments: below kChunkMinCap, pass 3 is stream_kernel
    s = gen.generate(2, n_docs=3, ops_per_doc=1400, mix=gen.MIX_INSERT, min_length=0)
    o, d = replay_both_cap(s, 1536)
    assert o.stats()["max_segs"] > 1534
    assert (d.statuses() == MTE_E_CAPACITY).all()
    assert_stopped_like_spec(s, d, 1536, streamed=True)


@pytest.mark.gpu
def test_gpu_stats_off_same_result():
    s = gen.generate(3, n_docs=80, ops_per_doc=2000)
    on = DeviceEngine(s["n_keys"])
    on.load_docs(s["inits"], s["init_text"])
    on.apply_batch(s["batch"])
    off = DeviceEngine(s["n_keys"])
    off.set_stats(False)
    off.load_docs(s["inits"], s["init_text"])
    off.apply_batch(s["batch"])
    np.testing.assert_array_equal(off.digest(), on.digest())
    np.testing.assert_array_equal(off.statuses(), on.statuses())
    assert on.stats()["ops_applied"] == int(s["batch"]["op_offsets"][-1])
    assert off.stats()["ops_applied"] == 0


@pytest.mark.gpu
def test_gpu_submit_rejects_bad_record():
    from fluidframework_amd.abi import MergeTreeError
    s = gen.generate(3, n_docs=40, ops_per_doc=3000)
    d = DeviceEngine(s["n_keys"])
    d.load_docs(s["inits"], s["init_text"])
    b = dict(s["batch"])
    ops = b["ops"].copy()
    ops["type"][77777] = 9  # one bad record deep inside the upload
    with pytest.raises(MergeTreeError) as e:
        d.submit(dict(b, ops=ops))
    assert "op 77777" in str(e.value)
    with pytest.raises(MergeTreeError):
        d.run()  # the failed submit discarded the batch
    d.apply_batch(s["batch"])  # a good batch still replays exactly
    o = SpecOracle(s["n_keys"], threads=8)
    o.load_docs(s["inits"], s["init_text"])
    o.apply_batch(s["batch"])
    np.testing.assert_array_equal(d.digest(), o.digest())


@pytest.mark.gpu
def test_gpu_paired_pass1_matches_oracle():
    # > CUs x 4 x 5 flat docs (MTE_PAIR_WAVES, mte_replay.h; `resident` in
    # mte_load_docs): pass 1 runs two documents per wave (alternating bursts);
    # smaller batches run one per wave.  length_mode 2: every document is flat
    # (of a default stream half are legacy and replay on the tree pass)
    s = gen.generate(3, n_docs=resident_docs() + 1, ops_per_doc=300, length_mode=2)
    o, d = replay_both(s, threads=16)
    assert (o.statuses() == 0).all()
    assert_same(o, d, sample_docs=24)


def test_gpu_fixtures_with_fresh_clients_every_round():
    # 512 distinct senders per document through 31 client slots (DocClients)
    passed, failures, eng = replay_fixtures(lambda k: DeviceEngine(k), fresh_clients=True)
    assert failures == []
    assert passed == 30 * 64 * 2
    _, _, oeng = replay_fixtures(lambda k: OracleEngine(k), check=False, fresh_clients=True)
    np.testing.assert_array_equal(eng.digest(), oeng.digest())


@pytest.mark.parametrize("cfg,round_sync", [(2, True), (3, False), (3, True), (4, False)])
def test_gpu_matches_oracle_at_full_bench_size(cfg, round_sync):
    # BASELINE configs 2 (1k docs x 1k ops), 3 (10k docs x 10k ops, the
    # headline) and 4 (100k docs x 500 ops) at full size: every document's
    # digest, status, op statistics and a sample of read-outs bit-exact against
    # the restatement.  round_sync: the streams bench.py times (legacy documents
    # declared MTE_DOC_ROUND_SYNC, on the flat passes behind the device check);
    # without it the legacy half replays on the tree pass
    s = gen.generate(cfg, **({"round_sync": True} if round_sync else {}))
    o, d = replay_both_cap(s, gen.seg_capacity(cfg, s["params"]), threads=16)
    assert (o.statuses() == 0).all()
    assert_same(o, d)


def test_gpu_pipelined_batches_equal_sequential():
    # mte_submit of batch k+1 while batch k replays (two batch slots, upload
    # stream): the same documents as one batch at a time with a sync between
    s = gen.generate(3, n_docs=300, ops_per_doc=1600, round_sync=True)
    parts = [gen.split_ops(s, k, 4) for k in range(4)] if hasattr(gen, "split_ops") else None
    if parts is None:
        pytest.skip("gen.split_ops missing")
    seq = DeviceEngine(s["n_keys"])
    gen.load_stream(seq, s)
    for p in parts:
        seq.submit(p)
        seq.run()
        seq.sync()
    pipe = DeviceEngine(s["n_keys"])
    gen.load_stream(pipe, s)
    for p in parts:
        pipe.submit(p)   # overlaps the previous run
        pipe.run()
    pipe.sync()
    np.testing.assert_array_equal(pipe.statuses(), seq.statuses())
    np.testing.assert_array_equal(pipe.digest(), seq.digest())
    o = SpecOracle(s["n_keys"], threads=8)
    gen.load_stream(o, s)
    o.apply_batch(s["batch"])
    np.testing.assert_array_equal(pipe.digest(), o.digest())
