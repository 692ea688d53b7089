"""The census of the walks that tests/test_gpu_state_walk.py makes, proved without a GPU and without a library call:
which pairs occur, that no step is a no-op, and that the counters have something to show."""
import math

import numpy as np
import pytest

from tests import builtin_probes
from tests import gauss_reference
from tests import state_walk as S

NAMES = list(S.FILTERS)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 15, 17])
def test_the_circuit_takes_every_edge_once(n):
    c = S.eulerian_circuit(n)
    edges = list(zip(c, c[1:]))
    assert len(edges) == n * n and len(set(edges)) == n * n
    assert set(edges) == {(a, b) for a in range(n) for b in range(n)}


@pytest.mark.parametrize("name", NAMES)
def test_every_ordered_pair_of_paths_occurs_exactly_once(name):
    paths, steps = S.paths_of(name), S.walk_of(name)
    assert steps[0].previous is None and steps[0].setter is None
    pairs = [(st.previous, st.path) for st in steps[1:]]
    assert len(pairs) == len(paths) ** 2 == len(set(pairs))
    assert set(pairs) == {(a, b) for a in paths for b in paths}
    assert [st.index for st in steps] == list(range(len(steps)))
    # consecutive steps are consecutive in the circuit
    assert all(a.path == b.previous for a, b in zip(steps, steps[1:]))


@pytest.mark.parametrize("name", NAMES)
def test_every_setter_stands_in_front_of_every_path(name):
    paths = S.paths_of(name)
    setters = S.filter_setters(name)
    assert len(paths) >= len(setters) + 1
    seen = {(st.setter, st.path) for st in S.walk_of(name)}
    assert {(s, p) for s in setters + [None] for p in paths} <= seen


def test_the_filters_take_the_setters_and_paths_that_apply():
    for name in NAMES:
        setters = S.filter_setters(name)
        assert ("native_input_frame" in setters) == S.FILTERS[name]["natives"]
        assert {"image_contents", "image_size", "image_sequence", "edge_colors", "sampling_offset", "render_size", "timing", "refused"} <= set(setters)
        assert bool(set(S.paths_of(name)) & set(S.NEEDS_SUPERSAMPLING)) == S.FILTERS[name]["options"].get("supersampling", False)
    assert set(S.paths_of("w1s")) == set(S.PATHS)                           # every path is walked: w1s takes all 17
    assert set(S.setters_of(S.new_model("w1"), False)) == set(S.SETTERS) - {"native_input_frame", "image_kind"}
    assert "image_kind" in S.filter_setters("w5")
    assert set(S.PATHS) == set(S.SINGLE_FRAME_PATHS) | set(S.CLIP_PATHS) and len(S.PATHS) == 17


@pytest.mark.parametrize("name", NAMES)
def test_every_setter_changes_what_the_model_sees_and_the_living_invocation_gets_one_change(name):
    model = S.new_model(name)
    for st in S.walk_of(name):
        if st.setter is None:
            continue
        before, ops_before = model.digest(), S.settings_ops(model)
        ops = S.change(model, st.setter)
        assert ops and model.digest() != before, st
        if st.setter != "refused":
            # ... and what apply() would replay has changed with it
            assert repr_ops(S.settings_ops(model)) != repr_ops(ops_before), st
        back = S.finish(model, st.setter)
        assert bool(back) == (st.setter == "render_size")
        assert model.render_size == model.canvas


def repr_ops(ops):
    return [(m, tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in args), sorted(kw.items())) for m, args, kw in ops]


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args, **kw: self.calls.append((name, args, kw))


def test_apply_replays_the_settings_and_only_the_settings():
    model = S.new_model("w1")
    for setter in S.setters_of(model, False):
        if setter != "refused":
            S.change(model, setter)
    rec = Recorder()
    S.apply(model, rec)
    names = [c[0] for c in rec.calls]
    assert not [n for n in names if n.startswith("render") or n == "sync"]
    assert names.count("set") == 4 and names.count("set_curve") == names.count("set_gradient") == names.count("set_image") == 1
    for once in ("set_edge_colors", "set_sampling_offset", "set_render_size", "set_native_input_frame", "enable_timing"):
        assert names.count(once) == 1, once
    image = [c for c in rec.calls if c[0] == "set_image"][0][1][1]
    assert image.shape == (S.SEQUENCE_FRAMES, S.IMAGE_OTHER[1], S.IMAGE_OTHER[0], 4) and image.dtype == np.uint8


@pytest.mark.parametrize("kind", S.IMAGE_KINDS)
def test_the_model_binds_every_kind_of_image(kind):
    model = S.new_model("w1")
    model.image = dict(kind=kind, size=S.IMAGE, frames=1 if kind == "uint8" else 3, seed=2)
    model.device = (0x1000, None)
    (method, args, kw), = S.image_ops(model)
    assert method == {"uint8": "set_image", "uint8_sequence": "set_image", "float32": "set_image", "device_uint32": "set_image_device",
                      "device_float": "set_image_device_float", "yuv420p": "set_image_yuv420", "yuv420p10": "set_image_yuv420p10"}[kind]
    if kind == "float32":
        assert args[1].dtype == np.float32 and args[1].min() < 0 and args[1].max() > 1
    if kind.startswith("yuv"):
        w, h = S.IMAGE
        assert args[1].shape == (3, w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)) and args[1].max() < (256 if kind == "yuv420p" else 1024)


def test_the_specialising_filter_sees_no_inexact_fold():
    """The literal folds of the specialising JIT ignore the sign of a zero and a non-finite value
    (builtin_probes.INEXACT_FOLD_SETS: "negzero", "nonfinite"): w2's user values are nonzero and finite."""
    assert builtin_probes.INEXACT_FOLD_SETS == ("negzero", "nonfinite")
    assert S.FILTERS["w2"]["options"]["specialize"] and S.FILTERS["w2"]["text"] == S.FILTERS["w1"]["text"]
    for name, (kind, values) in S.FILTERS["w2"]["scalars"].items():
        assert len(values) >= 2
        if kind in ("float", "int"):
            assert all(math.isfinite(v) and v != 0 for v in values), name
    # the walk returns to an earlier value set: every value is set more than once
    sets = []
    model = S.new_model("w2")
    for st in S.walk_of("w2"):
        if st.setter:
            S.change(model, st.setter)
            S.finish(model, st.setter)
        sets.append(tuple(sorted((k, v) for k, v in model.uservals.items() if k != "ca")))
    assert len(set(sets)) >= 4 and any(sets[i] != sets[i - 1] and sets[i] in sets[:i - 1] for i in range(2, len(sets)))


def test_the_blur_deviations_lie_on_both_sides_of_the_switch():
    for name in ("w3", "w3_edges", "w3_render", "w4"):
        fir = [gauss_reference.takes_fir(*gauss_reference.sigmas(S.CANVAS[0], S.CANVAS[1], s, s)) for s in S.FILTERS[name]["scalars"]["s"][1]]
        assert True in fir and False in fir, name


def test_the_image_is_smaller_than_the_canvas():
    assert S.IMAGE[0] < S.CANVAS[0] and S.IMAGE[1] < S.CANVAS[1] and S.IMAGE[0] < S.SMALL[0]
    # the other image is tall where the canvas is wide: render(in), which keeps the drawable's resize wrapper, leaves it
    assert S.IMAGE_OTHER[0] < S.CANVAS[0] and S.IMAGE_OTHER[1] > S.IMAGE_OTHER[0] and S.CANVAS[0] > S.CANVAS[1]
    assert S.SMALL[0] < S.CANVAS[0] and S.SMALL[1] < S.CANVAS[1]
    assert S.SMALL[0] % 2 and S.SMALL[1] % 2 and S.IMAGE[0] % 2 and S.IMAGE[1] % 2       # odd, no multiple of a tile


def simulate(name):
    """The counters the GPU test expects, from the model alone: (single-frame steps, predicted prologue skips, steps at
    which the memo must answer, steps at which it must not)."""
    spec, model = S.FILTERS[name], S.new_model(name)
    singles = skips = hits = misses = 0
    pkey = nkey = None
    for st in S.walk_of(name):
        if st.setter:
            S.change(model, st.setter)
        call = S.path_call(st.path, model, st.index)
        if st.path in S.SINGLE_FRAME_PATHS:
            singles += 1
            key, nat = S.prologue_key(call, model, spec["reads_t"]), model.native_key(call["frame"])
            skips += key == pkey
            if nkey is not None:
                hits += nat == nkey
                misses += nat != nkey
            pkey, nkey = key, nat
        else:
            pkey = nkey = None
        if st.setter:
            S.finish(model, st.setter)
    return singles, skips, hits, misses


@pytest.mark.parametrize("name", NAMES)
def test_the_counters_have_something_to_show(name):
    singles, skips, hits, misses = simulate(name)
    paths = S.paths_of(name)
    assert singles == len(paths) * len(set(paths) & set(S.SINGLE_FRAME_PATHS)) + (1 if S.walk_of(name)[0].path in S.SINGLE_FRAME_PATHS else 0)
    if S.FILTERS[name]["natives"]:
        assert hits >= 1 and misses >= 3, (hits, misses)
    else:
        assert 1 <= skips < singles, skips


def test_the_deep_walk_binds_every_kind_of_image():
    model, kinds = S.new_model("w5"), set()
    for st in S.walk_of("w5"):
        if st.setter:
            S.change(model, st.setter)
            S.finish(model, st.setter)
        kinds.add((model.image["kind"], model.image["frames"] > 1, st.path))
    for kind in S.IMAGE_KINDS:
        seen = {p for k, _, p in kinds if k == kind}
        assert seen & set(S.SINGLE_FRAME_PATHS) and seen & set(S.CLIP_PATHS), kind
    assert {(k, seq) for k, seq, _ in kinds} >= {(k, True) for k in S.KIND_CYCLE[:5]} | {(k, False) for k in S.KIND_CYCLE}


def test_which_prologues_read_t():
    """The model's `reads_t` is the generator's: a read of t (a plain in(xy) makes one) is hoisted into the prologue.
    (Compiles the filters: the front end alone, no GPU.)"""
    import re
    import mathmap_amd as mm
    for name in ("w1", "w1t", "w2"):
        ir = mm.Filter(S.FILTERS[name]["text"], **S.FILTERS[name]["options"]).ir_json
        reads = bool(re.search(r'"rhs":\{"k":"internal","name":"(t|frame)"\},"hoisted":1', ir))
        assert reads == S.FILTERS[name]["reads_t"], name


def test_chunks_keep_the_order():
    steps = S.walk_of("w1")
    parts = S.chunks(steps, 5)
    assert len(parts) == 5 and [st for part in parts for st in part] == steps
