"""One device sink through chains of stages, on nine and more chunks (csrc/mesher.hip: simplifyChunks, stageInPlace,
stageIntoNewGeneration, the normals cache, the kept reference, dense and output chunk numbers; mlsgpu::seamMask in
csrc/fill.hip).  The model of sink_chain_cases.py starts from the chunks the sink serves behind finalize() and runs every
stage's oracle beside the device: after every step the sink's chunks are the model's through the stage's own assert_same --
every vertex bit, every triangle row, every statistic --, and at the steps marked R every report is the oracle's for the
model's chunks.  tests/test_sink_chain_oracle.py shows on the CPU that the inputs have what these chains need."""
import numpy as np
import pytest

import compact_cases as cpc
import deviation_cases as dc
import intersect_cases as ic
import normals_cases as nc
import sink_chain_cases as k
import topology_cases as tc
from gpu_common import ctx  # noqa: F401
from sink_cases import mo

pytestmark = pytest.mark.gpu


class Chain:
    """A finalized sink of one variant of the sheet and its model, stepped together."""

    def __init__(self, ctx, name, tmp_path):
        import mlsgpu_amd as m
        from mlsgpu_amd import binding as b
        self.b, self.tmp_path = b, tmp_path
        meshes, prune = k.variant(name)
        self.mesher = m.Mesher(ctx, prune)
        for mesh in meshes:                                         # the caller's ids as they are: not dense, not monotonic
            self.mesher.add(mesh["chunk"], mesh["vertices"], mesh["num_internal"], mesh["keys"], mesh["triangles"])
        want, want_stats = mo.mesh_sink(meshes, prune)
        self.count = self.mesher.finalize()
        self.finalize_stats = self.mesher.stats()
        got = [self.mesher.chunk(i) for i in range(self.count)]
        assert [(c["chunk"], len(c["vertices"]), len(c["triangles"])) for c in got] == [(c, len(v), len(t)) for c, v, t in want]
        assert all(self.finalize_stats[key] == want_stats[key] for key in want_stats)
        self.model = k.SinkModel.from_output([(c["chunk"], c["vertices"], c["triangles"]) for c in got], k.quiet_chunks(meshes, prune))
        self.simplified = False
        self.assert_seams_closed("finalize")

    def chunks(self):
        return [self.mesher.chunk(i) for i in range(self.count)]

    def assert_seams_closed(self, step):
        if not self.simplified:
            assert k.open_seams([(c["chunk"], c["vertices"], c["triangles"]) for c in self.chunks()]) == [], step

    def assert_chunks(self, step, stage=True):
        """The sink's output chunks are the model's: count, ids, bytes, and behind a stage the oracle's result through the stage's
        assert_same (stage=False: no stage ran); the normals of every chunk are the oracle's for the model's chunk; stats() is
        finalize's."""
        want = self.model.chunks()
        assert len(want) == self.count
        for i, (cid, v, t) in enumerate(want):
            c = self.mesher.chunk(i)
            assert c["chunk"] == cid and (c["num_vertices"], c["num_triangles"]) == (len(v), len(t)), (step, i)
            result = self.model.last[self.model.out[i]]
            if stage and result is not None:
                k.assert_chunk(step, c["vertices"], c["triangles"], result)
            assert c["vertices"].tobytes() == v.tobytes() and c["triangles"].tobytes() == t.tobytes(), (step, i)
            got = self.mesher.chunk_normals(i)
            nc.assert_same((got["normals"], got["stats"]), nc.normals(v, t))
        assert self.mesher.stats() == self.finalize_stats, step

    def assert_reports(self, step):
        b = self.b
        for i, (_, v, t) in enumerate(self.model.chunks()):
            assert tc.report_fields(self.mesher.chunk_topology(i)) == tc.count_all(len(v), t), (step, i)
            self.mesher.write_ply(i, self.tmp_path / "device.ply", comments=(step,))
            b.write_ply(self.tmp_path / "host.ply", v, t, comments=(step,))
            assert (self.tmp_path / "device.ply").read_bytes() == (self.tmp_path / "host.ply").read_bytes(), (step, i)
            blob, st = self.mesher.chunk_compact(i, 32)
            dv, dt = cpc.decode(blob)
            assert (st["numVertices"], st["numTriangles"]) == (len(v), len(t)), (step, i)
            assert np.asarray(dv, np.float32).tobytes() == v.tobytes() and np.asarray(dt, np.uint32).tobytes() == t.tobytes(), (step, i)
        ic.same_stats(self.mesher.self_intersections(), self.model.self_intersections())
        self.assert_deviation()

    def assert_deviation(self):
        if self.model.reference is None:
            with pytest.raises(self.b.InvalidArgument):
                self.mesher.deviation(k.DEVIATION)
            return
        moved, lost = self.mesher.deviation(k.DEVIATION)
        want_moved, want_lost = self.model.deviation(k.DEVIATION)
        dc.same_stats(moved, want_moved)
        dc.same_stats(lost, want_lost)

    def step(self, name, args=(), reports=False):
        for i in (0, 4):                                            # computed before the step: must not be served after it
            self.mesher.chunk_normals(i)
        want = getattr(self.model, name)(*args)
        got = getattr(self.mesher, name)(*args)
        if name == "finalize":
            assert got == want == self.count
        elif name != "keep_reference":
            assert got == want, (name, got, want)
        self.simplified = (self.simplified or name.startswith("simplify")) and name != "finalize"
        self.assert_chunks(name, stage=name not in ("keep_reference", "finalize"))
        self.assert_seams_closed(name)
        if reports:
            self.assert_reports(name)

    def run(self, steps, reports=True):
        for name, args, r in steps:
            self.step(name, args, r and reports)

    def close(self):
        self.mesher.close()


@pytest.mark.parametrize("name", ["tiles", "gaps", "twins"])
def test_grow_and_shrink(ctx, tmp_path, name):  # noqa: F811
    """S1: keep_reference, fill R, split R, collapse, flip, smooth R, split, keep_reference, collapse R, finalize -- the originals
    bit for bit, the reference still kept, the deviation against it the model's --, then fill to smooth again with the same bits
    as the first time.  `gaps`: eleven dense chunks, nine with output, ids neither dense nor monotonic; the chunk without
    triangles pins the corners of a hole of tile 4 for the first fill and is gone from the mask after it.  `twins`: a run of the
    seam mask that one chunk enters twice, with and without a neighbour's copy, and -0.0 beside +0.0."""
    chain = Chain(ctx, name, tmp_path)
    assert chain.count == 9 and len(chain.model.dense) == (11 if name == "gaps" else 9)
    first = {}
    for n, (step, args, r) in enumerate(k.S1):
        chain.step(step, args, r and n < 10)                        # the reports once: the second time repeats the bits
        if step == "finalize":
            chain.assert_deviation()                                # against the reference of step 8, kept across the finalize
            moved, _ = chain.mesher.deviation(k.DEVIATION)
            assert moved["numPoints"] == sum(len(d[1]) for d in chain.model.dense)
        if 1 <= n <= 5 or n >= 10:                                  # steps 2 to 6, the first and the second time
            first.setdefault(step, []).append([(c["vertices"].tobytes(), c["triangles"].tobytes()) for c in chain.chunks()])
    assert all(len(runs) == 2 and runs[0] == runs[1] for runs in first.values()) and len(first) == 5
    chain.close()


@pytest.mark.parametrize("name", ["tiles", "crumb"])
def test_to_the_front_and_on(ctx, tmp_path, name):  # noqa: F811
    """S2: simplify R, repair, repair with split pinches R, fill -- the mask has the stray coincidences and the repair's twins --,
    flip, split R, quadric simplify, collapse R.  On `crumb` the tenth chunk is empty from the simplify on: chunk(9) and every
    report on it are what the mesh-level function makes of the empty mesh."""
    chain = Chain(ctx, name, tmp_path)
    assert chain.count == (10 if name == "crumb" else 9)
    for step, args, r in k.S2:
        chain.step(step, args, r)
        if name == "crumb" and step != "keep_reference":
            c = chain.mesher.chunk(9)
            assert (c["chunk"], c["num_vertices"], c["num_triangles"]) == (9, 0, 0)
    chain.close()


def test_everything_emptied(ctx, tmp_path):  # noqa: F811
    """S3: a simplify cell larger than the sheet leaves nine chunks without a vertex; every other stage once and every report on
    them; finalize brings the originals back."""
    chain = Chain(ctx, "tiles", tmp_path)
    for step, args, r in k.S3:
        chain.step(step, args, r)
        if step not in ("keep_reference", "finalize"):
            assert all(c["num_vertices"] == 0 and c["num_triangles"] == 0 for c in chain.chunks())
    assert sum(c["num_triangles"] for c in chain.chunks()) == 2 * (48 * 48 - len(k.HOLES))
    chain.close()


def test_refusals_inside_a_chain(ctx, tmp_path):  # noqa: F811
    """S4: between the split and the collapse of S1 one refused parameter per stage, a split that max_growth = 1 gives no room,
    and a deviation after drop_reference: the chunks are the model's before and after, and the chain goes on to S1's bits."""
    chain = Chain(ctx, "tiles", tmp_path)
    b, mesher = chain.b, chain.mesher
    chain.run(k.S1[:3], reports=False)
    refused = [lambda: mesher.simplify(k.SIMPLIFY_ORIGIN, 0.0), lambda: mesher.simplify_quadric(k.SIMPLIFY_ORIGIN, -1.0),
               lambda: mesher.smooth(3, lam=0.0), lambda: mesher.flip_edges(k.MAX_ROUNDS, min_gain=-1.0), lambda: mesher.fill_holes(2),
               lambda: mesher.repair(2), lambda: mesher.collapse_edges(k.MAX_ROUNDS, -1.0), lambda: mesher.split_edges(k.MAX_ROUNDS, 0.0)]
    for call in refused:
        for i in (0, 4):
            mesher.chunk_normals(i)
        with pytest.raises(b.InvalidArgument):
            call()
        chain.assert_chunks("refused", stage=False)
    chain.step("split_edges", (k.MAX_ROUNDS, k.SPLIT_LENGTH, 1))
    chain.assert_deviation()
    mesher.drop_reference()
    chain.model.drop_reference()
    chain.assert_deviation()                                        # refused: nothing is kept
    chain.assert_chunks("refused", stage=False)
    chain.run(k.S1[3:10], reports=False)
    chain.close()
