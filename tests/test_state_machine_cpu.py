"""The animation state machine and blend-tree nodes of the shim: sequencing only, no pose arithmetic. Scripted updates
are checked through the layer's runtime state and the pose program each update emits; every expected value is worked
out here from the reference's rules (AnimationStateMachine.cpp:242-504, AnimationBlendTree.cpp:38-229) in float32."""
import numpy as np
import pytest

import anim_cases
import anim_graph_ref as G
import anim_ref
from trident_raster import abi, app, raster

F = np.float32
NO = G.NO_MASK
IDLE, WALK, RUN, STILL = 0, 1, 2, 3
DUR = {IDLE: F(1.0), WALK: F(2.0), RUN: F(0.5), STILL: F(0.0)}


def _key(bone, x):
    return {"bone": bone, "T": (np.array([0.0], F), np.array([[x, 0.0, 0.0]], F)), "R": None, "S": None}


@pytest.fixture(scope="module")
def asset():
    """Two bones and four clips that differ in duration: idle 1 s, walk 2 s, run 0.5 s, still 0 s."""
    lb = np.stack([anim_ref.compose([0.5, 0, 0], [1, 0, 0, 0], [1, 1, 1]), anim_ref.compose([0, 0.25, 0], [1, 0, 0, 0], [1, 1, 1])])
    ib = np.stack([anim_ref.compose([0, 0, 0], [1, 0, 0, 0], [1, 1, 1])] * 2)
    rig = anim_ref.Rig("sm_rig", [-1, 0], lb.astype(F), ib.astype(F))
    rig.clips = [anim_ref.Clip("idle", 1.0, [_key(0, 1.0)]), anim_ref.Clip("walk", 2.0, [_key(0, 2.0)]),
                 anim_ref.Clip("run", 0.5, [_key(1, 3.0)]), anim_ref.Clip("still", 0.0, [_key(1, 4.0)])]
    h, clips = anim_cases.cpu_asset(rig)
    assert clips == [IDLE, WALK, RUN, STILL]
    return h


def _machine(asset, states=("idle", "walk"), entry="idle"):
    """One override layer whose states play the clip of their name (looping, speed 1)."""
    sm = app.StateMachine(asset)
    layer = sm.add_layer("base")
    for name in states:
        sm.add_state(layer, name, app.node_clip({"idle": IDLE, "walk": WALK, "run": RUN, "still": STILL}[name]))
    if entry:
        sm.set_layer_entry(layer, entry)
    return sm


def _acc(*steps):
    """Float32 accumulation, as the machine's timers add up."""
    t = F(0.0)
    for s in steps:
        t = F(t + F(s))
    return float(t)


def _loop(t, clip):
    m = np.fmod(F(t), DUR[clip])
    return float(F(DUR[clip] + m) if m < 0 else m)


def test_entry_state_on_the_first_update_and_the_program(asset):
    with _machine(asset) as sm:
        assert sm.layer_state(0)[:2] == ("", "")
        assert sm.program() == ([], [])
        sm.update(0.25)
        assert sm.layer_state(0) == ("idle", "", 0.25, 0.0, 0.0)
        # the final pose starts at rest; the layer's clip; the layer's blend at weight 1 (an all-ones mask: no mask)
        assert sm.program() == ([(G.REST, 0, 0.0), (G.CLIP, IDLE, 0.25), (G.BLEND, NO, 1.0)], [])
        assert np.array_equal(sm.pose(), app.anim_eval_program(asset, sm.program()[0]))
        assert np.array_equal(sm.pose(), app.anim_evaluate(asset, IDLE, 0.25))  # blend at F = 1 of exact values


def test_no_layers_no_entry_state_and_a_missing_clip(asset):
    with app.StateMachine(asset) as sm:
        sm.update(0.1)
        assert sm.program() == ([(G.REST, 0, 0.0)], [])
        assert np.array_equal(sm.pose(), app.anim_evaluate(asset, None, 0.0))
    with _machine(asset, entry=None) as sm:  # no entry state: the layer holds the rest pose and never starts
        sm.update(0.1)
        assert sm.layer_state(0) == ("", "", 0.0, 0.0, 0.0)
        assert sm.program()[0] == [(G.REST, 0, 0.0), (G.REST, 0, 0.0), (G.BLEND, NO, 1.0)]
    with app.StateMachine(asset) as sm:  # a clip node whose clip is missing yields the rest pose
        layer = sm.add_layer("base")
        sm.add_state(layer, "ghost", app.node_clip(77))
        sm.set_layer_entry(layer, "ghost")
        sm.update(0.1)
        assert sm.program()[0] == [(G.REST, 0, 0.0), (G.REST, 0, 0.0), (G.BLEND, NO, 1.0)]
    with app.StateMachine(None) as sm:  # no skeleton: nothing happens
        sm.add_layer("base")
        sm.update(0.1)
        assert sm.program() == ([], []) and sm.pose().shape == (0, 16)


def test_exit_time_gates_a_transition(asset):
    with _machine(asset) as sm:
        sm.add_transition(0, "idle", "walk", fade=0.2, exit_time=0.5)
        sm.update(0.2)
        sm.update(0.2)
        assert sm.layer_state(0)[:3] == ("idle", "", _acc(0.2, 0.2))
        sm.update(0.2)  # 0.6 >= 0.5
        assert sm.layer_state(0) == ("idle", "walk", _acc(0.2, 0.2, 0.2), 0.0, float(F(0.2)))


CASES = [
    # (parameter type, value, comparison, condition value, taken)
    (app.SM_FLOAT, 1.5, "==", 1.5, True), (app.SM_FLOAT, 1.5, "==", 1.6, False), (app.SM_FLOAT, 1.5, "!=", 1.6, True),
    (app.SM_FLOAT, 1.5, "!=", 1.5, False), (app.SM_FLOAT, 1.5, ">", 1.0, True), (app.SM_FLOAT, 1.5, ">", 1.5, False),
    (app.SM_FLOAT, 1.5, "<", 2.0, True), (app.SM_FLOAT, 1.5, "<", 1.5, False), (app.SM_FLOAT, 1.5, ">=", 1.5, True),
    (app.SM_FLOAT, 1.5, ">=", 1.6, False), (app.SM_FLOAT, 1.5, "<=", 1.5, True), (app.SM_FLOAT, 1.5, "<=", 1.4, False),
    # integers compare as integers for == / != (the condition's int value) and as floats for the orderings
    (app.SM_INTEGER, 3, "==", 3, True), (app.SM_INTEGER, 3, "==", 4, False), (app.SM_INTEGER, 3, "!=", 4, True),
    (app.SM_INTEGER, 3, "!=", 3, False), (app.SM_INTEGER, 3, ">", 2, True), (app.SM_INTEGER, 3, "<", 3, False),
    (app.SM_INTEGER, 3, ">=", 3, True), (app.SM_INTEGER, 3, "<=", 2, False),
    # bools compare with the condition's bool for == / != and as 1.0 / 0.0 for the orderings
    (app.SM_BOOL, 1, "==", True, True), (app.SM_BOOL, 1, "==", False, False), (app.SM_BOOL, 0, "!=", True, True),
    (app.SM_BOOL, 0, "!=", False, False), (app.SM_BOOL, 1, ">", 0.5, True), (app.SM_BOOL, 0, ">=", 0.5, False),
    # a trigger: Triggered consumes it; == sees it as 1.0 / 0.0 and leaves it
    (app.SM_TRIGGER, 1, "triggered", 0, True), (app.SM_TRIGGER, 0, "triggered", 0, False),
    (app.SM_TRIGGER, 1, "==", 1.0, True), (app.SM_TRIGGER, 1, "<", 0.5, False),
    # Triggered on a parameter that is no trigger never holds
    (app.SM_FLOAT, 1.0, "triggered", 0, False),
]


@pytest.mark.parametrize("kind,value,cmp_,against,taken", CASES)
def test_each_comparison_on_each_parameter_type(asset, kind, value, cmp_, against, taken):
    with _machine(asset) as sm:
        sm.add_parameter("p", kind, value)
        if kind == app.SM_TRIGGER and value:
            sm.fire("p")
        sm.add_transition(0, "idle", "walk", fade=0.0, conditions=[("p", cmp_, against)])
        sm.update(0.1)
        assert sm.layer_state(0)[0] == ("walk" if taken else "idle")
    with _machine(asset) as sm:  # a condition on a parameter the machine does not have fails
        sm.add_transition(0, "idle", "walk", fade=0.0, conditions=[("absent", cmp_, against)])
        sm.update(0.1)
        assert sm.layer_state(0)[0] == "idle" and sm.parameter("absent") is None


def test_parameter_conversions(asset):
    with _machine(asset) as sm:
        sm.add_parameter("f", app.SM_FLOAT, 2.75)
        sm.add_parameter("i", app.SM_INTEGER, -3)
        sm.add_parameter("b", app.SM_BOOL, 1)
        sm.add_parameter("t", app.SM_TRIGGER)
        assert sm.parameter("f") == (app.SM_FLOAT, 2.75, False)
        assert sm.parameter("i") == (app.SM_INTEGER, -3.0, False)
        assert sm.parameter("b") == (app.SM_BOOL, 1.0, False)
        assert sm.parameter("t") == (app.SM_TRIGGER, 0.0, False)
        sm.fire("t")
        assert sm.parameter("t") == (app.SM_TRIGGER, 1.0, True)
        sm.reset_trigger("t")
        assert sm.parameter("t") == (app.SM_TRIGGER, 0.0, False)
        sm.set_parameter("f", app.SM_INTEGER, 7)  # a set changes the type, as in the reference
        assert sm.parameter("f") == (app.SM_INTEGER, 7.0, False)
        sm.fire("new")  # FireTrigger creates the parameter
        assert sm.parameter("new") == (app.SM_TRIGGER, 1.0, True)


def test_a_trigger_is_consumed_once_and_also_by_a_transition_that_fails(asset):
    with _machine(asset, states=("idle", "walk", "run")) as sm:
        sm.add_parameter("go", app.SM_TRIGGER)
        sm.add_parameter("flag", app.SM_BOOL, 0)
        # the first transition reaches its Triggered condition, consumes the trigger, then fails on the flag; the second
        # finds the trigger gone
        sm.add_transition(0, "idle", "walk", fade=0.0, conditions=[("go", "triggered", 0), ("flag", "==", True)])
        sm.add_transition(0, "idle", "run", fade=0.0, conditions=[("go", "triggered", 0)])
        sm.fire("go")
        sm.update(0.1)
        assert sm.layer_state(0)[0] == "idle" and sm.parameter("go")[2] is False
        sm.update(0.1)
        assert sm.layer_state(0)[0] == "idle"
        # with the flag's condition in front, the failing transition never reaches the trigger: the second takes it
    with _machine(asset, states=("idle", "walk", "run")) as sm:
        sm.add_parameter("go", app.SM_TRIGGER)
        sm.add_parameter("flag", app.SM_BOOL, 0)
        sm.add_transition(0, "idle", "walk", fade=0.0, conditions=[("flag", "==", True), ("go", "triggered", 0)])
        sm.add_transition(0, "idle", "run", fade=0.0, conditions=[("go", "triggered", 0)])
        sm.fire("go")
        sm.update(0.1)
        assert sm.layer_state(0)[0] == "run" and sm.parameter("go")[2] is False
        sm.update(0.1)  # consumed once: run has no way back, and nothing fires again
        assert sm.layer_state(0)[0] == "run"


def test_a_fade_its_completion_and_the_target_reset(asset):
    dt, fade = 0.05, 0.2
    with _machine(asset, states=("idle", "walk", "run")) as sm:
        sm.add_parameter("go", app.SM_TRIGGER)
        sm.add_parameter("r", app.SM_TRIGGER)
        sm.add_transition(0, "idle", "walk", fade=fade, conditions=[("go", "triggered", 0)])
        sm.add_transition(0, "idle", "run", fade=fade, conditions=[("r", "triggered", 0)])
        sm.add_transition(0, "walk", "idle", fade=fade, conditions=[("go", "triggered", 0)])
        sm.update(dt)
        sm.update(dt)
        sm.fire("go")
        sm.update(dt)  # the transition starts: elapsed 0, the target reset and advanced by this update's dt
        idle_t = _acc(dt, dt, dt)
        assert sm.layer_state(0) == ("idle", "walk", idle_t, 0.0, float(F(fade)))
        assert sm.program()[0] == [(G.REST, 0, 0.0), (G.CLIP, IDLE, idle_t), (G.CLIP, WALK, _acc(dt)), (G.BLEND, NO, 0.0),
                                   (G.BLEND, NO, 1.0)]
        sm.fire("r")  # a transition is in flight: the scan does not run, and the trigger stays
        elapsed, walk_t = F(0.0), F(dt)
        for _ in range(3):
            sm.update(dt)
            elapsed, walk_t, idle_t = F(elapsed + F(dt)), F(walk_t + F(dt)), _acc(idle_t, dt)
            assert elapsed < F(fade)
            assert sm.layer_state(0) == ("idle", "walk", idle_t, float(elapsed), float(F(fade)))
            T = float(F(elapsed) / F(fade))
            assert sm.program()[0][2:4] == [(G.CLIP, WALK, float(walk_t)), (G.BLEND, NO, T)]
        assert sm.parameter("r")[2] is True
        sm.update(dt)  # elapsed reaches the duration: walk is current, its time in state restarts, its clip goes on
        assert F(elapsed + F(dt)) >= F(fade)
        assert sm.layer_state(0) == ("walk", "", 0.0, 0.0, 0.0)
        assert sm.program()[0] == [(G.REST, 0, 0.0), (G.CLIP, WALK, float(F(walk_t + F(dt)))), (G.BLEND, NO, 1.0)]
        # back to idle: its clip was at idle_t and restarts from 0 (Reset of the target's root), plus this update's dt
        sm.fire("go")
        sm.update(dt)
        assert sm.layer_state(0)[:2] == ("walk", "idle")
        assert sm.program()[0][2] == (G.CLIP, IDLE, _acc(dt))


def test_a_zero_duration_transition_snaps(asset):
    with _machine(asset) as sm:
        sm.add_parameter("go", app.SM_TRIGGER)
        sm.add_transition(0, "idle", "walk", fade=0.0, conditions=[("go", "triggered", 0)])
        sm.update(0.3)
        sm.fire("go")
        sm.update(0.1)
        assert sm.layer_state(0) == ("walk", "", 0.0, 0.0, 0.0)
        assert sm.program()[0] == [(G.REST, 0, 0.0), (G.CLIP, WALK, _acc(0.1)), (G.BLEND, NO, 1.0)]


def test_a_transition_to_a_missing_state_is_skipped_and_an_unknown_source_is_an_error(asset):
    with _machine(asset) as sm:
        sm.add_parameter("go", app.SM_TRIGGER)
        sm.add_transition(0, "idle", "nowhere", fade=0.0, conditions=[("go", "triggered", 0)])
        sm.fire("go")
        sm.update(0.1)
        assert sm.layer_state(0)[:2] == ("idle", "") and sm.parameter("go")[2] is False  # conditions ran first
        with pytest.raises(raster.TriError) as e:
            sm.add_transition(0, "nowhere", "idle")
        assert e.value.code == abi.TRI_E_STATE  # AddTransition's std::runtime_error


def test_both_children_of_a_blend_node_advance(asset):
    with app.StateMachine(asset) as sm:
        layer = sm.add_layer("base")
        sm.add_parameter("w", app.SM_FLOAT, 0.25)
        sm.add_state(layer, "mix", app.node_blend(app.node_clip(IDLE), app.node_clip(WALK, speed=2.0), 0.75, "w"))
        sm.set_layer_entry(layer, "mix")
        sm.update(0.125)
        sm.update(0.125)
        assert sm.program()[0] == [(G.REST, 0, 0.0), (G.CLIP, IDLE, 0.25), (G.CLIP, WALK, 0.5), (G.BLEND, NO, 0.25),
                                   (G.BLEND, NO, 1.0)]
        sm.set_parameter("w", app.SM_FLOAT, 7.0)  # the node clamps its weight
        sm.update(0.0)
        assert sm.program()[0][3] == (G.BLEND, NO, 1.0)
    with app.StateMachine(asset) as sm:  # without a second child: the first child's pose; without a first: empty
        layer = sm.add_layer("base")
        sm.add_state(layer, "half", app.node_blend(app.node_clip(IDLE), None))
        sm.add_state(layer, "none", app.node_blend(None, app.node_clip(WALK)))
        sm.add_state(layer, "bare", app.node_blend(None, None))
        sm.add_parameter("n", app.SM_TRIGGER)
        sm.add_transition(layer, "half", "none", fade=0.0, conditions=[("n", "triggered", 0)])
        sm.add_transition(layer, "none", "bare", fade=0.0, conditions=[("n", "triggered", 0)])
        sm.set_layer_entry(layer, "half")
        sm.update(0.25)
        assert sm.program()[0] == [(G.REST, 0, 0.0), (G.CLIP, IDLE, 0.25), (G.BLEND, NO, 1.0)]
        for _ in range(2):  # an empty layer pose: the layer's blend runs over no bones and is folded away
            sm.fire("n")
            sm.update(0.25)
            assert sm.program() == ([(G.REST, 0, 0.0)], [])


def test_clip_time_loops_clamps_and_follows_a_speed_parameter(asset):
    def times(node, steps):
        with app.StateMachine(asset) as sm:
            layer = sm.add_layer("base")
            sm.add_parameter("spd", app.SM_FLOAT, 2.0)
            sm.add_state(layer, "s", node)
            sm.set_layer_entry(layer, "s")
            out = []
            for dt in steps:
                sm.update(dt)
                out.append(sm.program()[0][1][2])
            return out

    steps = [0.375, 0.375, 0.375]
    t, want = F(0.0), []
    for dt in steps:  # looping: fmod into [0, duration)
        t = F(_loop(F(t + F(dt)), IDLE))
        want.append(float(t))
    assert times(app.node_clip(IDLE), steps) == want == [0.375, 0.75, 0.125]
    t, want = F(0.0), []
    for dt in steps:  # negative speed: a negative remainder wraps to the end
        t = F(_loop(F(t + F(dt) * F(-1.0)), IDLE))
        want.append(float(t))
    assert times(app.node_clip(IDLE, speed=-1.0), steps) == want == [0.625, 0.25, 0.875]
    assert times(app.node_clip(RUN, looping=False), steps) == [0.375, 0.5, 0.5]            # clamped at the duration
    assert times(app.node_clip(RUN, looping=False, speed=-1.0), steps) == [0.0, 0.0, 0.0]  # ... and at 0
    assert times(app.node_clip(STILL, looping=True), steps) == [0.375, 0.75, 1.125]        # duration 0: neither
    assert times(app.node_clip(STILL, looping=False, speed=-1.0), steps) == [-0.375, -0.75, -1.125]
    assert times(app.node_clip(WALK, speed_parameter="spd"), steps) == [0.75, 1.5, 0.25]   # the parameter overrides
    assert times(app.node_clip(WALK, speed=0.5, speed_parameter="absent"), steps) == [0.1875, 0.375, 0.5625]


def test_blend_space_neighbours(asset):
    def at(samples, p, steps=(0.75, 0.75)):
        with app.StateMachine(asset) as sm:
            layer = sm.add_layer("base")
            sm.add_parameter("p", app.SM_FLOAT, p)
            sm.add_state(layer, "s", app.node_blend_space(samples, 0.0, "p"))
            sm.set_layer_entry(layer, "s")
            for dt in steps:
                sm.update(dt)
            return sm.program()[0][1:-1]

    samples = [(RUN, 2.0), (IDLE, 0.0), (WALK, 1.0)]  # sorted by position on construction
    t = 1.5  # the node's time only grows: past idle's and run's durations, never wrapped
    assert at(samples, -1.0) == [(G.CLIP, IDLE, t), (G.CLIP, RUN, t), (G.BLEND, NO, 0.0)]   # below: first and last
    assert at(samples, 0.25) == [(G.CLIP, IDLE, t), (G.CLIP, WALK, t), (G.BLEND, NO, 0.25)]
    assert at(samples, 1.5) == [(G.CLIP, WALK, t), (G.CLIP, RUN, t), (G.BLEND, NO, 0.5)]
    assert at(samples, 1.0) == [(G.CLIP, IDLE, t), (G.CLIP, WALK, t), (G.BLEND, NO, 1.0)]   # the first pair that brackets
    assert at(samples, 3.0) == [(G.CLIP, IDLE, t), (G.CLIP, RUN, t), (G.BLEND, NO, 1.0)]    # above: first and last, clamped
    # equal positions keep the order they were given in (a stable sort), and their pair divides by eps
    equal = [(RUN, 1.0), (WALK, 1.0), (IDLE, 0.0)]
    assert at(equal, 1.0) == [(G.CLIP, IDLE, t), (G.CLIP, RUN, t), (G.BLEND, NO, 1.0)]
    assert at([(RUN, 1.0), (WALK, 1.0)], 1.0) == [(G.CLIP, RUN, t), (G.CLIP, WALK, t), (G.BLEND, NO, 0.0)]
    assert at([(WALK, 1.0), (RUN, 1.0)], 1.0) == [(G.CLIP, WALK, t), (G.CLIP, RUN, t), (G.BLEND, NO, 0.0)]
    assert at([(WALK, 1.0)], 5.0) == [(G.CLIP, WALK, t), (G.CLIP, WALK, t), (G.BLEND, NO, 1.0)]
    assert at([(WALK, 1.0), (None, 2.0)], 1.5) == [(G.REST, 0, 0.0)]  # a missing clip: the rest pose
    with app.StateMachine(asset) as sm:  # no samples: the empty pose
        layer = sm.add_layer("base")
        sm.add_state(layer, "s", app.node_blend_space([], 0.0))
        sm.set_layer_entry(layer, "s")
        sm.update(0.1)
        assert sm.program() == ([(G.REST, 0, 0.0)], [])


def test_three_small_machines_emit_these_programs(asset):
    # 1: one layer, one clip state, a half-weight layer with a mask shorter than the skeleton (padded with 1.0)
    with _machine(asset) as sm:
        sm.set_layer_weight(0, 0.5)
        sm.set_layer_mask(0, [0.25])
        sm.update(0.5)
        ops, masks = sm.program()
        assert ops == [(G.REST, 0, 0.0), (G.CLIP, IDLE, 0.5), (G.BLEND, 0, 0.5)]
        assert [m.tolist() for m in masks] == [[0.25, 1.0]]
        sm.set_layer_mask(0, [1.0, 1.0, 0.0])  # longer: truncated to the bones, and all ones is no mask
        sm.update(0.0)
        assert sm.program() == ([(G.REST, 0, 0.0), (G.CLIP, IDLE, 0.5), (G.BLEND, NO, 0.5)], [])
    # 2: an override layer mid-fade under an additive masked layer driven by a blend space
    with _machine(asset) as sm:
        sm.add_parameter("go", app.SM_TRIGGER)
        sm.add_parameter("lean", app.SM_FLOAT, 0.5)
        sm.add_transition(0, "idle", "walk", fade=0.5, conditions=[("go", "triggered", 0)])
        upper = sm.add_layer("upper", 0.75, additive=True)
        sm.add_state(upper, "lean", app.node_blend_space([(RUN, 0.0), (STILL, 2.0)], 0.0, "lean"))
        sm.set_layer_entry(upper, "lean")
        sm.set_layer_mask(upper, [0.0, 1.0])
        sm.fire("go")
        sm.update(0.25)
        sm.update(0.125)
        ops, masks = sm.program()
        assert ops == [(G.REST, 0, 0.0),
                       (G.CLIP, IDLE, 0.375), (G.CLIP, WALK, 0.375), (G.BLEND, NO, 0.25), (G.BLEND, NO, 1.0),
                       (G.CLIP, RUN, 0.375), (G.CLIP, STILL, 0.375), (G.BLEND, NO, 0.25), (G.ADD, 0, 0.75)]
        assert [m.tolist() for m in masks] == [[0.0, 1.0]]
        assert np.array_equal(sm.pose(), app.anim_eval_program(asset, ops, masks))
    # 3: a layer without an entry state under a layer whose state has no root node: two rest poses
    with app.StateMachine(asset) as sm:
        sm.add_layer("a", 0.5)
        b = sm.add_layer("b", 2.0, additive=True)
        sm.add_state(b, "rootless", None)
        sm.set_layer_entry(b, "rootless")
        sm.update(0.1)
        assert sm.program() == ([(G.REST, 0, 0.0), (G.REST, 0, 0.0), (G.BLEND, NO, 0.5), (G.REST, 0, 0.0), (G.ADD, NO, 2.0)], [])
        assert sm.layer_state(b)[0] == "rootless"


def test_a_skeleton_handle_that_goes_away_between_updates(asset):
    with _machine(asset) as sm:
        sm.update(0.25)
        before, program = sm.pose(), sm.program()
        sm.set_handles(None, None)
        sm.update(0.25)  # no skeleton: no change at all, timers included
        assert np.array_equal(sm.pose(), before) and sm.program() == program
        assert sm.layer_state(0)[2] == 0.25
        sm.set_handles(asset, asset)
        sm.update(0.25)
        assert sm.program()[0][1] == (G.CLIP, IDLE, 0.5)


def test_the_animation_system_drives_a_component_state_machine(asset):
    """UpdateComponent with a state machine: the component's handles, dt or 0 when not playing, the pose copied;
    InitialisePose updates by 0."""
    a = app.TridentApp()
    try:
        e = a.add_mesh_entity("cube")
        a.set_entity_animation(e, "test:sm_rig", "test:sm_rig", "run", time=0.0)
        with app.StateMachine(None) as sm:  # the system hands it the component's handles
            layer = sm.add_layer("base")
            sm.add_state(layer, "idle", app.node_clip(IDLE))
            sm.set_layer_entry(layer, "idle")
            a.set_entity_state_machine(e, sm)
            a.initialise_pose(e)  # Update(0): the entry state at time 0
            assert sm.layer_state(0)[:3] == ("idle", "", 0.0)
            assert np.array_equal(a.entity_pose(e), sm.pose()) and sm.pose().shape == (2, 16)
            a.update_animation(0.25)
            assert sm.program()[0][1] == (G.CLIP, IDLE, 0.25)
            assert np.array_equal(a.entity_pose(e), app.anim_eval_program(asset, sm.program()[0]))
            assert a.entity_animation_state(e)[0] == 0.0  # the clip fields are not what plays
            a.set_entity_animation(e, "test:sm_rig", "test:sm_rig", "run", playing=False)
            a.update_animation(0.25)  # m_IsPlaying false: the machine updates by 0
            assert sm.program()[0][1] == (G.CLIP, IDLE, 0.25) and sm.layer_state(0)[2] == 0.25
            a.set_device_pose(True)  # the system only advances now; the pose on demand is the program's CPU evaluation
            a.set_entity_animation(e, "test:sm_rig", "test:sm_rig", "run", playing=True)
            a.update_animation(0.25)
            assert sm.program()[0][1] == (G.CLIP, IDLE, 0.5)
            assert np.array_equal(a.entity_pose(e), sm.pose())
            a.set_entity_state_machine(e, None)
    finally:
        a.close()
