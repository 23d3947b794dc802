"""Entity ids through the engine API on the GPU: Renderer::PickEntity, PickEntitiesInRect, ReadViewportEntityIds and
SetSelectionOutline over three mesh entities (one hidden) and a sprite in two viewports, with frames in flight, and on
multi-device viewports (ids yes, outline refused).

The expected entity of every pixel comes from the frame's own inputs (trident_app_frame_inputs + the concatenated
geometry) through tests/id_ref.py's reference, mapped through the draw table the shim documents: visible mesh entities
in registry order, then sprites."""
import numpy as np
import pytest

import id_ref

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
CLEAR = (0.1, 0.2, 0.3, 1.0)
VIEWPORTS = {1: (100, 70), 2: (90, 60)}  # the editor camera's and the runtime camera's


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def make_app(app_mod, viewports=VIEWPORTS):
    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 1.0, 7.0), far=60.0)
    a.set_camera("runtime", (0.8, 1.4, 6.0), (0.0, 6.0, 0.0), far=60.0)
    for vp, (w, h) in viewports.items():
        a.set_viewport(vp, w, h)
    a.set_clear_color(CLEAR)
    ents = {
        "cube": a.add_mesh_entity("cube", position=(-1.4, 1.0, -1.0), rotation=(20.0, 30.0, 0.0), scale=(1.6, 1.6, 1.6)),
        "hidden": a.add_mesh_entity("cube", position=(0.0, 1.0, 1.0), scale=(1.0, 1.0, 1.0)),
        "sphere": a.add_mesh_entity("sphere", position=(1.3, 1.2, 0.0), scale=(1.8, 1.8, 1.8)),
        # (the sprite quad faces away from a camera on +z until it is turned round)
        "sprite": a.add_sprite_entity(position=(0.0, 0.2, 1.5), rotation=(0.0, 180.0, 0.0), scale=(1.2, 0.8, 1.0),
                                      tint=(0.9, 0.4, 0.2, 1.0)),
    }
    a.set_entity_visible(ents["hidden"], False)
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
    return a, ents


def expected_entities(a, oracle, vp, ents, background=NONE, size=None, names=("cube", "sphere", "sprite")):
    """(entity image, expected ids, draw table) of the viewport's next frame, from its inputs. names: the entities the
    frame draws, in draw order."""
    from trident_raster import scenes

    w, h = size or VIEWPORTS[vp]
    ubo, draws = a.frame_inputs(vp)
    vb, ib, ranges = a.geometry()
    s = scenes.Scene(f"shim_vp{vp}", w, h, vb, ib, ranges, draws, ubo, materials=[(m[0], m[1]) for m in a.materials()],
                     clear=CLEAR)
    ids, _ = id_ref.expected_ids(oracle, s)
    table = [ents[n] for n in names]  # visible meshes in registry order, then sprites
    assert len(draws) == len(table)
    image = np.full(ids.shape, background, np.uint32)
    for d, e in enumerate(table):
        image[ids == d + 1] = e
    return image, ids, table


def a_pixel_of(image, value):
    ys, xs = np.nonzero(image == value)
    assert ys.size, value
    k = ys.size // 2
    return int(xs[k]), int(ys[k])


def test_pick_and_entity_image_in_two_viewports(app_mod, oracle):
    a, ents = make_app(app_mod)
    a.draw_frame()
    assert a.read_entity_ids(1, *VIEWPORTS[1]) is None and a.pick_entity(1, 50, 35) is None  # no ids asked for yet
    for vp in VIEWPORTS:
        a.set_entity_id_output(vp, True)
    want = {vp: expected_entities(a, oracle, vp, ents) for vp in VIEWPORTS}
    a.draw_frame()
    for vp, (w, h) in VIEWPORTS.items():
        image, ids, table = want[vp]
        got = a.read_entity_ids(vp, w, h)
        bad = int((got != image).sum())
        print(f"SHIM viewport {vp}: {bad} entity mismatches, entities {np.unique(image).tolist()}")
        assert bad == 0
        assert ents["hidden"] not in got and set(table) <= set(np.unique(got).tolist())
        _, depth = a.read_pixels(vp, w, h)
        for e in table:
            x, y = a_pixel_of(image, e)
            assert a.pick_entity(vp, x, y) == (e, float(depth[y, x])), (vp, e, x, y)
        x, y = a_pixel_of(image, NONE)
        assert a.pick_entity(vp, x, y) is None  # background
        for x, y in [(-1, 0), (w, 0), (0, h)]:
            assert a.pick_entity(vp, x, y) is None
        assert a.pick_entities_in_rect(vp, 0, 0, w - 1, h - 1) == table  # every entity, in draw order
        x, y = a_pixel_of(image, ents["sphere"])
        assert a.pick_entities_in_rect(vp, x, y, x, y) == [ents["sphere"]]
        box = image[10:31, 20:61]
        inside = [e for e in table if (box == e).any()]
        assert a.pick_entities_in_rect(vp, 20, 10, 60, 30) == inside
        assert np.array_equal(a.read_entity_ids(vp, w, h, background=7), np.where(image == NONE, 7, image))
    assert a.pick_entity(9, 1, 1) is None and a.read_entity_ids(9, 4, 4) is None  # no such viewport
    a.set_entity_id_output(2, False)
    a.draw_frame()
    assert a.read_entity_ids(2, *VIEWPORTS[2]) is None and a.read_entity_ids(1, *VIEWPORTS[1]) is not None
    a.close()


def test_pick_with_three_frames_in_flight(app_mod, oracle):
    """Each ring target is a context of its own with its own id image and draw table: the readers answer for the latest
    frame, whichever target it went to."""
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    a.set_frames_in_flight(3)
    a.set_entity_id_output(1, True)
    w, h = VIEWPORTS[1]
    for k in range(5):
        a.set_entity_transform(ents["cube"], position=(-1.4 + 0.5 * k, 1.0, -1.0))
        if k == 3:
            a.set_entity_visible(ents["hidden"], True)  # another draw list: the table of this target changes
        names = ("cube", "hidden", "sphere", "sprite") if k == 3 else ("cube", "sphere", "sprite")
        image, ids, table = expected_entities(a, oracle, 1, ents, names=names)
        a.draw_frame()
        got = a.read_entity_ids(1, w, h)
        assert int((got != image).sum()) == 0, k
        assert (ents["hidden"] in got) == (k == 3)
        assert a.pick_entities_in_rect(1, 0, 0, w - 1, h - 1) == table, k
        if k == 3:
            a.set_entity_visible(ents["hidden"], False)
        x, y = a_pixel_of(image, ents["cube"])
        assert a.pick_entity(1, x, y)[0] == ents["cube"], k
    a.close()


def test_selection_outline_changes_only_outline_pixels(app_mod, oracle):
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    w, h = VIEWPORTS[1]
    image, ids, table = expected_entities(a, oracle, 1, ents)
    a.draw_frame()
    base, _ = a.read_pixels(1, w, h)
    assert a.read_entity_ids(1, w, h) is None
    colour = (1.0, 0.6, 0.0, 1.0)
    a.set_selected_entity(ents["sphere"])
    assert a.set_selection_outline(True, colour, 2)
    a.draw_frame()
    lined, _ = a.read_pixels(1, w, h)
    assert np.array_equal(a.read_entity_ids(1, w, h), image)  # the outline turned the id output on
    mask = id_ref.outline_mask(ids, [table.index(ents["sphere"])], 2)
    want = base.copy()
    want[mask] = id_ref.colour_bytes(colour)[[2, 1, 0, 3]]  # (read_pixels is RGBA)
    bad = int((lined != want).any(axis=-1).sum())
    print(f"SHIM outline: {int(mask.sum())} outline pixels, {bad} wrong")
    assert mask.sum() > 50 and bad == 0
    a.set_selected_entity(ents["hidden"])  # selected, not drawn: nothing to outline
    a.draw_frame()
    assert np.array_equal(a.read_pixels(1, w, h)[0], base)
    a.set_selected_entity(ents["sprite"])
    a.draw_frame()
    mask = id_ref.outline_mask(ids, [table.index(ents["sprite"])], 2)
    want = base.copy()
    want[mask] = id_ref.colour_bytes(colour)[[2, 1, 0, 3]]
    assert mask.any() and np.array_equal(a.read_pixels(1, w, h)[0], want)
    assert not a.set_selection_outline(True, colour, 9)  # refused: the width-2 outline stays
    a.draw_frame()
    assert np.array_equal(a.read_pixels(1, w, h)[0], want)
    assert a.set_selection_outline(False)
    a.draw_frame()
    assert np.array_equal(a.read_pixels(1, w, h)[0], base)
    a.close()


@pytest.mark.parametrize("inflight", [1, 3])
def test_ids_and_outline_survive_a_viewport_resize(app_mod, oracle, inflight):
    """A resize replaces the viewport's context (every ring target's, each when its turn comes): the id output and the
    outline are set again on the new one, so the next frame picks, reads ids and draws the outline as before."""
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    a.set_frames_in_flight(inflight)
    colour = (0.2, 0.9, 1.0, 1.0)
    a.set_entity_id_output(1, True)
    a.set_selected_entity(ents["cube"])
    assert a.set_selection_outline(True, colour, 3)
    for _ in range(inflight):  # every ring target has rendered with ids and the outline
        a.draw_frame()
    assert a.read_entity_ids(1, *VIEWPORTS[1]) is not None
    for size in [(120, 90), (80, 50)]:
        w, h = size
        a.set_viewport(1, w, h)
        image, ids, table = expected_entities(a, oracle, 1, ents, size=size)
        for k in range(inflight):  # each target's first frame at the new size
            a.draw_frame()
            got = a.read_entity_ids(1, w, h)
            assert got is not None and int((got != image).sum()) == 0, (size, k)
            x, y = a_pixel_of(image, ents["sphere"])
            assert a.pick_entity(1, x, y)[0] == ents["sphere"], (size, k)
            assert a.pick_entities_in_rect(1, 0, 0, w - 1, h - 1) == table, (size, k)
            lined, _ = a.read_pixels(1, w, h)
            mask = id_ref.outline_mask(ids, [table.index(ents["cube"])], 3)
            assert mask.sum() > 30
            assert (lined[mask] == id_ref.colour_bytes(colour)[[2, 1, 0, 3]]).all(), (size, k)
        assert a.set_selection_outline(False)
        a.draw_frame()
        plain, _ = a.read_pixels(1, w, h)
        assert np.array_equal(plain[~mask], lined[~mask]) and not (plain[mask] == lined[mask]).all(axis=-1).any()
        assert a.set_selection_outline(True, colour, 3)
    a.close()


def test_multi_device_viewports_have_ids_but_no_outline(app_mod, oracle, capfd):
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    w, h = VIEWPORTS[1]
    a.set_selected_entity(ents["cube"])
    assert a.set_selection_outline(True)
    capfd.readouterr()
    a.set_device_count(2, [0, 0])  # turns the outline off, and says so
    assert "selection outline" in capfd.readouterr().err
    a.set_entity_id_output(1, True)
    image, ids, table = expected_entities(a, oracle, 1, ents)
    a.draw_frame()
    base, depth = a.read_pixels(1, w, h)
    assert not a.set_selection_outline(True)  # refused, with a log line
    assert "selection outline" in capfd.readouterr().err
    a.draw_frame()
    assert np.array_equal(a.read_pixels(1, w, h)[0], base)
    assert int((a.read_entity_ids(1, w, h) != image).sum()) == 0
    x, y = a_pixel_of(image, ents["cube"])
    assert a.pick_entity(1, x, y) == (ents["cube"], float(depth[y, x]))
    assert a.pick_entities_in_rect(1, 0, 0, w - 1, h - 1) == table
    a.close()
