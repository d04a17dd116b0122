"""What the ray-query tests share (closest hit, segment any-hit, hit lists): the batch sizes, and device_query_contract's World
with the scene's model objects, the oracle's scene and shuffled rays on the device and the host.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import numpy as np

import device_query_contract as dq
from device_query_contract import BATCHES  # noqa: F401 (the one definition; the ray-query modules take it from here)
import intersect_reference as ref
import segment_reference as seg
from oracle import binding as ob

CLOSEST_ALL = ("hit_id", "t", "hit_point", "normal")
INF = np.float32(np.inf)
N_MODEL = 2000   # rays of the comparisons with the oracle's per-object test (the CPU suite's set)
N_MESH = 515     # rays on the triangle mesh: eight blocks and three lanes


class World(dq.World):
    """The shared World (host scene, device scenes by tree, each with its grid) with the model objects, the oracle's scene and
    max(BATCHES) shuffled rays on the device and the host"""

    def __init__(self, path, trees, seed=8, n=max(BATCHES), oracle=True):
        super().__init__(path, trees, grid=True)
        self.objs = ref.load_objects(path)
        self.sc = ob.Scene(path) if oracle else None
        o, d = ref.scene_rays(self.objs, seed, n)
        order = np.random.default_rng(seed + 100).permutation(len(o))  # every prefix holds aimed and random rays
        self.set_rays(o[order], d[order])

    def set_rays(self, o, d):
        self.attach(d_origin=np.ascontiguousarray(o, np.float32), d_direction=np.ascontiguousarray(d, np.float32))
        self.o, self.d, self.d_o, self.d_d = self.host["d_origin"], self.host["d_direction"], self.dev["d_origin"], self.dev["d_direction"]
        self._tests = self._table = None

    @property
    def tests(self):
        """The oracle's per-object answers for the first N_MODEL rays"""
        if self._tests is None:
            self._tests = seg.per_object(self.sc.object_intercepts, len(self.objs), self.o[:N_MODEL], self.d[:N_MODEL])
        return self._tests

    def table(self, n):
        """The model's per-object answers for the first n rays"""
        if self._table is None or self._table[0].shape[1] < n:
            self._table = ref._all(self.objs, self.o[:n], self.d[:n])
        return tuple(a[:, :n] for a in self._table)


def limit_sets(w, n):
    """name -> n limits: the seeded draws of the CPU suite, and the ties: the nearest of the oracle's hits, its two
    neighbours (1 where nothing is hit), then 0, inf and NaN"""
    t_near, has = seg.nearest(w.tests)
    same, up, down = seg.tie_limits(np.where(has, t_near, np.float32(1)))
    sets = {"draws": seg.draw_limits(w.objs, w.o[:n], w.d[:n], 18, table=w.table(n)), "t itself": same, "the float above t": up,
            "the float below t": down, "zero": np.zeros(n, np.float32), "inf": np.full(n, INF), "NaN": np.full(n, np.nan, np.float32)}
    return sets, has
