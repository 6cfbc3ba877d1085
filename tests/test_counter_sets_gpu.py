"""The step pipeline's rotation of counter sets: two lanes, and three counter sets -- or two, option
"counter_sets" -- that consecutive counts take in turn.  Seven steps take every (lane, set) pairing and come round to the
first again; every test runs at both numbers of sets.  Need an MI355X: python -m pytest tests -m gpu."""
import numpy as np
import pytest

import lesseq_amd as L

pytestmark = pytest.mark.gpu

SETS = (3, 2)
STEPS = 7


def make_ctx(ev, reads, sets, **options):
    ctx = L.Context(0)
    ctx.set_option("counter_sets", sets)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.upload_events(ev)
    ctx.upload_reads(0, reads)
    return ctx


def device_tables(ctx, ev):
    """three device buffers of a step's own, filled with ones' bits so that a hand-off that never came shows"""
    import torch
    n_cls = int(L.lib.lsq_results_num_classes(ctx.h))
    return (torch.full((n_cls,), -1, dtype=torch.int64, device="cuda:0"), torch.full((ev.total_isoforms,), -1.0, dtype=torch.float64, device="cuda:0"),
            torch.full((len(ev),), -1.0, dtype=torch.float64, device="cuda:0"))


def handed_over(ctx, bufs):
    ctx.copy_results_device(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr())


def same_tables(a, b):
    # (bit for bit: the log-likelihood of an event without reads may be a NaN, which equals only its own bits)
    return all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


def to_host(bufs):
    return tuple(b.cpu().numpy() for b in bufs)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """about 200 mixed events and three read sets of 20-50 k reads over them, and per read set what ONE synchronous step of a fresh
    context gives: the handed-over tables, counts() and solution().  Computed once; the tests only read it."""
    import torch
    d = tmp_path_factory.mktemp("counter_sets")
    specs = [L.SynthSpec(60 + i, 200, n, 100, 2, L.EVENT_TYPES) for i, n in enumerate((30000, 50000, 20000))]
    L.synth_write(specs[0], str(d), "p", write_mrf=False)
    ann = L.Annotation(str(d / "p.interval"), str(d / "p.map"))
    ev = L.Events(ann, ("SHORT_READ",), (100,))
    # (the annotation is that of specs[0]; the other read sets lie over other annotations of the same chromosomes: what falls on these events counts)
    reads = [L.Reads.synthetic(sp, ev) for sp in specs]
    ref = []
    for r in reads:
        ctx = make_ctx(ev, r, 3)
        ctx.count(); ctx.solve()
        bufs = device_tables(ctx, ev)
        torch.cuda.synchronize()
        handed_over(ctx, bufs)
        ctx.synchronize()
        ref.append(dict(tables=to_host(bufs), counts=[x.copy() for x in ctx.counts()], solution=[x.copy() for x in ctx.solution()]))
        ctx.close()
    assert int(ref[0]["counts"][0].sum()) > 1000 and int(ref[0]["tables"][0].sum()) == int(ref[0]["counts"][0].sum())
    assert len({int(r["counts"][0].sum()) for r in ref}) == 3          # three read sets that differ
    return dict(ev=ev, reads=reads, ref=ref)


def same_host_results(ctx, want):
    cnt, bases = ctx.counts()
    if not (np.array_equal(cnt, want["counts"][0]) and np.array_equal(bases, want["counts"][1])):
        return False
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ctx.solution(), want["solution"]))


@pytest.mark.parametrize("sets", SETS)
def test_seven_steps_back_to_back_each_with_tables_of_its_own(job, sets):
    """seven steps submitted without waiting, each handing its tables to buffers of its own: every one equal to a synchronous step's.
    Then seven more with the read set changing from step to step."""
    import torch
    ev, reads, ref = job["ev"], job["reads"], job["ref"]
    ctx = make_ctx(ev, reads[0], sets)
    outs = [device_tables(ctx, ev) for _ in range(2 * STEPS)]
    torch.cuda.synchronize()             # torch's fills run on torch's stream, the hand-offs on the library's
    for k in range(STEPS):
        ctx.count(); ctx.solve()
        handed_over(ctx, outs[k])
    which = [(k + 1) % 3 for k in range(STEPS)]
    for k, i in enumerate(which):
        ctx.upload_reads(0, reads[i])
        ctx.count(); ctx.solve()
        handed_over(ctx, outs[STEPS + k])
    ctx.synchronize()
    for k in range(STEPS):
        assert same_tables(to_host(outs[k]), ref[0]["tables"]), "step %d" % k
    for k, i in enumerate(which):
        assert same_tables(to_host(outs[STEPS + k]), ref[i]["tables"]), "step %d with read set %d" % (k, i)
    assert same_host_results(ctx, ref[which[-1]])
    ctx.close()


@pytest.fixture(scope="module")
def tie_job(tmp_path_factory):
    """the input of test_exception_list_overflow_is_settled_on_the_device: reads that cover an event's span exactly, so that many
    (read, event) pairs go through the exception list; its whole tables from a list that is large enough"""
    import golden_inputs as gi
    d = tmp_path_factory.mktemp("counter_sets_ties")
    info = gi.write_events_case(str(d), "x", seed=77, n_events=40, n_reads=3000, R=60, n_chrom=2)
    lines = open(d / "x.mrf").read().split("\n")
    extra = []
    for e in info["events"]:
        gs = min(f[0][0] for f in e["forms"]); ge = max(f[-1][1] for f in e["forms"])
        for strand in ("+", "-", e["strand"]):
            extra.append("%s:%s:%d:%d:1:%d" % (e["chrom"], strand, gs + 1, ge, ge - gs))
    with open(d / "x.mrf", "w") as f:
        f.write("\n".join(lines[:-1] + extra) + "\n")
    ann = L.Annotation(str(d / "x.interval"), str(d / "x.map"), 0, 1000)
    ev = L.Events(ann, ("SHORT_READ",), (60,))
    reads = L.Reads.from_mrf(str(d / "x.mrf"), ev)
    import torch
    ctx = make_ctx(ev, reads, 3)
    ctx.count(); ctx.solve()
    pairs, recounted = ctx.count_status()
    assert recounted == [0] and pairs[0] > 7
    bufs = device_tables(ctx, ev)
    torch.cuda.synchronize()
    handed_over(ctx, bufs)
    ctx.synchronize()
    out = dict(ev=ev, reads=reads, tables=to_host(bufs), pairs=pairs)
    ctx.close()
    return out


@pytest.mark.parametrize("sets", SETS)
def test_seven_steps_with_an_exception_list_that_overflows(tie_job, sets):
    """the same with a 7-entry exception list: every count ends in the recount, on the device, and every handed-over table is whole;
    lsq_count_status reports the latest count"""
    import torch
    ev, reads = tie_job["ev"], tie_job["reads"]
    ctx = make_ctx(ev, reads, sets, exception_capacity=7)
    outs = [device_tables(ctx, ev) for _ in range(STEPS)]
    torch.cuda.synchronize()
    for b in outs:
        ctx.count(); ctx.solve()
        handed_over(ctx, b)
    ctx.synchronize()
    for k, b in enumerate(outs):
        assert same_tables(to_host(b), tie_job["tables"]), "step %d" % k
    # the pairs of THIS count (as many as the large list took: every pair is counted, kept or not) and its flag
    assert ctx.count_status() == (tie_job["pairs"], [1])
    # ... and of the next one, which counts every read again because it is told to, its list large enough or not
    ctx.set_option("recount_every_read", 1)
    ctx.count()
    assert ctx.count_status() == (tie_job["pairs"], [1])
    ctx.set_option("recount_every_read", 0)
    ctx.close()
    ctx = make_ctx(ev, reads, sets)
    for k in range(STEPS):
        ctx.count(); ctx.solve()
        if k == 2:
            ctx.set_option("recount_every_read", 1)      # steps 3 .. 5 recount, the last one does not: the status is the last one's
        if k == 5:
            ctx.set_option("recount_every_read", 0)
    assert ctx.count_status() == (tie_job["pairs"], [0])
    ctx.close()


@pytest.mark.parametrize("sets", SETS)
def test_counts_without_solves_in_between(job, sets):
    """k = 1 .. 7 counts and one solve behind the last (k = 2: count, count, solve), and seven counts with no solve at all: the
    zeroing of a set does not depend on a solve having been queued"""
    ev, reads, ref = job["ev"], job["reads"], job["ref"]
    for k in range(1, STEPS + 1):
        ctx = make_ctx(ev, reads[0], sets)
        for _ in range(k):
            ctx.count()
        ctx.solve()
        assert same_host_results(ctx, ref[0]), "%d counts, then a solve" % k
        ctx.close()
    ctx = make_ctx(ev, reads[0], sets)
    for _ in range(STEPS):
        ctx.count()
    cnt, bases = ctx.counts()
    assert np.array_equal(cnt, ref[0]["counts"][0]) and np.array_equal(bases, ref[0]["counts"][1])
    ctx.close()


@pytest.mark.parametrize("sets", SETS)
def test_counts_set_by_the_caller_are_what_the_em_reads(job, sets):
    """lsq_results_set_counts + solve after 1, 2 and 3 earlier steps: the solution of those counts, as a context that never counted
    gives it; and the counts that come back are the ones that were set"""
    ev, reads, ref = job["ev"], job["reads"], job["ref"]
    cnt, bases = 3 * ref[1]["counts"][0] + 1, 3 * ref[1]["counts"][1] + 100          # (no read set of the job gives these)
    fresh = make_ctx(ev, reads[0], sets)
    fresh.set_counts(cnt, bases)
    fresh.solve()
    want = dict(counts=[cnt, bases], solution=[x.copy() for x in fresh.solution()])
    fresh.close()
    assert not np.array_equal(want["solution"][0], ref[0]["solution"][0])
    for earlier in (1, 2, 3):
        ctx = make_ctx(ev, reads[0], sets)
        for _ in range(earlier):
            ctx.count(); ctx.solve()
        ctx.set_counts(cnt, bases)
        ctx.solve()
        assert same_host_results(ctx, want), "after %d steps" % earlier
        ctx.count(); ctx.solve()          # ... and the next count starts from zeroed counters, not from what was set
        assert same_host_results(ctx, ref[0]), "the step after, after %d steps" % earlier
        ctx.close()


@pytest.mark.parametrize("sets", SETS)
def test_switching_the_number_of_sets_between_steps(job, sets):
    """"counter_sets" changed on a context whose streams have drained, after 1, 2 and 3 steps (every set the latest once), then seven
    steps: the same tables.  With work in flight the option is refused."""
    import torch
    ev, reads, ref = job["ev"], job["reads"], job["ref"]
    other = 5 - sets
    ctx = make_ctx(ev, reads[0], sets)
    now = sets
    for before in (1, 2, 3, 1):
        for _ in range(before):
            ctx.count(); ctx.solve()
        ctx.synchronize()
        now = other if now == sets else sets
        ctx.set_option("counter_sets", now)
        outs = [device_tables(ctx, ev) for _ in range(STEPS)]
        torch.cuda.synchronize()
        for b in outs:
            ctx.count(); ctx.solve()
            handed_over(ctx, b)
        ctx.synchronize()
        for k, b in enumerate(outs):
            assert same_tables(to_host(b), ref[0]["tables"]), "step %d at %d sets, switched after %d steps" % (k, now, before)
    with pytest.raises(L.LsqError):
        ctx.set_option("counter_sets", 4)
    # in flight: the latest lane's result stream is held behind an event of a stream that spins for some tens of milliseconds, and the
    # zeroing that the next count queues on it cannot run
    side = torch.cuda.Stream()
    held = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(5_000_000)
        held.record(side)
    torch.cuda.ExternalStream(ctx.result_stream, device=torch.device("cuda", 0)).wait_event(held)
    ctx.count(); ctx.solve()
    with pytest.raises(L.LsqError):
        ctx.set_option("counter_sets", other if now == sets else sets)
    ctx.synchronize()
    assert same_host_results(ctx, ref[0])
    ctx.set_option("counter_sets", other if now == sets else sets)
    ctx.count(); ctx.solve()
    assert same_host_results(ctx, ref[0])
    ctx.close()
