"""Integration tests driving the in-tree headless Wayland compositor
through a REAL protocol client (unix socket, wire format, SCM_RIGHTS
fds): registry/globals, shm surfaces + xdg toplevels, seat input
injection, output management and data-device clipboard."""

import os

import pytest

from selkies_amd.wayland import compositor as wcomp
from selkies_amd.wayland.client import WaylandClient
from selkies_amd.wayland.compositor import Compositor


@pytest.fixture()
def comp(sock_dir, monkeypatch):
    monkeypatch.setenv("XDG_RUNTIME_DIR", str(sock_dir))
    c = Compositor(f"selkies-test-{os.getpid()}", 1280, 720)
    c.start()
    yield c
    c.stop()


def test_registry_and_outputs(comp):
    cli = WaylandClient(comp.display_name)
    try:
        assert "wl_compositor" in cli.globals
        assert "wl_seat" in cli.globals
        assert "xdg_wm_base" in cli.globals
        assert "wl_data_device_manager" in cli.globals
        assert len(cli.outputs) == 1
        info = next(iter(cli.outputs.values()))
        assert info["mode"][1:3] == [1280, 720]
    finally:
        cli.close()


def test_window_map_and_list(comp):
    cli = WaylandClient(comp.display_name)
    try:
        cli.map_window(400, 300, title="editor")
        cli.roundtrip()
        wins = comp.list_windows()
        assert len(wins) == 1
        assert wins[0]["title"] == "editor"
        assert (wins[0]["width"], wins[0]["height"]) == (400, 300)
        assert wins[0]["focused"]
        # the committed shm buffer composites into the capture frame
        w, h, fb = comp.composite_frame()
        assert (w, h) == (1280, 720)
        assert fb[0] == 0x42
    finally:
        cli.close()


def test_inject_key_reaches_seat(comp):
    cli = WaylandClient(comp.display_name)
    try:
        cli.setup_seat()
        assert cli.keymap and "xkb_keymap" in cli.keymap
        assert cli.keymap == comp.get_xkb_keymap_string()
        cli.map_window()
        comp.inject_key(30, True)    # KEY_A
        comp.inject_key(30, False)
        cli.pump(1.0)
        keys = cli.key_events()
        assert [(k[2], k[3]) for k in keys] == [(30, 1), (30, 0)]
    finally:
        cli.close()


def test_inject_pointer(comp):
    cli = WaylandClient(comp.display_name)
    try:
        cli.setup_seat()
        cli.map_window()
        comp.inject_mouse_move(100.5, 50.25)
        comp.inject_mouse_button(0x110, True)   # BTN_LEFT
        comp.inject_mouse_button(0x110, False)
        comp.inject_mouse_scroll(0, 15.0)
        cli.pump(1.0)
        motions = cli.pointer_events("motion")
        assert motions and motions[-1][1][1:] == [100.5, 50.25]
        buttons = [a for n, a in cli.pointer_events("button")]
        assert [(b[2], b[3]) for b in buttons] == [(0x110, 1), (0x110, 0)]
        axes = cli.pointer_events("axis")
        assert axes and axes[0][1][2] == 15.0
    finally:
        cli.close()


def test_output_management(comp):
    cli = WaylandClient(comp.display_name)
    try:
        name = comp.create_output(800, 600, x=1280, y=0)
        cli.pump(1.0)
        assert len(cli.outputs) == 2
        assert len(comp.list_outputs()) == 2
        geo = comp.get_realized_geometry()
        assert geo["width"] == 1280 + 800
        assert comp.reposition_output(name, 0, 720)
        assert comp.get_realized_geometry()["height"] == 720 + 600
        assert comp.destroy_output(name)
        assert len(comp.list_outputs()) == 1
    finally:
        cli.close()


def test_clipboard_compositor_to_app(comp):
    cli = WaylandClient(comp.display_name)
    try:
        cli.setup_seat()
        cli.map_window()
        cli.setup_data_device()
        comp.set_clipboard("hello wayland")
        cli.pump(1.0)
        assert "text/plain;charset=utf-8" in cli.selection_mimes
        assert cli.read_selection() == b"hello wayland"
    finally:
        cli.close()


def test_clipboard_app_to_compositor(comp):
    cli = WaylandClient(comp.display_name)
    try:
        cli.setup_seat()
        cli.map_window()
        cli.setup_data_device()
        cli.set_selection(b"from-the-app")
        cli.pump(0.3)
        assert comp.clipboard_types_app() == ["text/plain;charset=utf-8"]
        got = [None]
        import threading
        t = threading.Thread(
            target=lambda: got.__setitem__(0, comp.clipboard_read_app()))
        t.start()
        for _ in range(100):
            cli.pump(0.05)
            if not t.is_alive():
                break
        t.join(timeout=2)
        assert got[0] == b"from-the-app"
    finally:
        cli.close()


def test_ensure_wayland_display_idempotent(sock_dir, monkeypatch):
    monkeypatch.setenv("XDG_RUNTIME_DIR", str(sock_dir))
    name = wcomp.ensure_wayland_display(f"selkies-ew-{os.getpid()}")
    try:
        assert wcomp.get_wayland_display_name() == name
        assert wcomp.ensure_wayland_display("other-name") == name
        cli = WaylandClient(name)
        assert "wl_compositor" in cli.globals
        cli.close()
    finally:
        wcomp.shutdown_wayland_display()
        assert wcomp.get_wayland_display_name() is None


def test_input_dispatcher_wayland_backend(comp, monkeypatch):
    """The wire-protocol dispatcher drives the Wayland seat end to end:
    'kd,<keysym>' arrives at a real client as wl_keyboard.key."""
    from selkies_amd import wayland as wmod
    from selkies_amd.input_handler import InputDispatcher, make_backend
    monkeypatch.setattr(wmod.compositor, "_compositor", comp)
    cli = WaylandClient(comp.display_name)
    try:
        cli.setup_seat()
        cli.map_window()
        backend = make_backend("wayland-0")
        disp = InputDispatcher(backend, enable_input=True)
        disp.on_message("kd,97")    # 'a'
        disp.on_message("ku,97")
        disp.on_message("m,10,20")
        cli.pump(1.0)
        keys = cli.key_events()
        assert [(k[2], k[3]) for k in keys] == [(30, 1), (30, 0)]  # KEY_A
        assert cli.pointer_events("motion")
    finally:
        cli.close()


def test_shm_publisher_feeds_native_engine(comp, tmp_path):
    """End-to-end capture seam: client commits a buffer -> compositor
    composites -> seqlock shm file -> native engine 'shm:' backend
    encodes it -> decoded luma shows the client's pixels (the reference
    use_wayland capture contract, engine-side)."""
    import struct as _st
    import threading

    import numpy as np

    hipflux = pytest.importorskip("hipflux")
    if not hipflux.native_available():
        pytest.skip("native module not built")
    from hipflux import _native
    from h264_ref_decoder import Decoder

    cli = WaylandClient(comp.display_name)
    try:
        cli.map_window(1280, 720, title="fb")
        cli.roundtrip()
        path = str(tmp_path / "fb.shm")
        comp.start_shm_publisher(path, fps=30)
        try:
            # wait until a stable (even, nonzero) seq is published
            deadline = 5.0
            import time as _t
            t0 = _t.time()
            while _t.time() - t0 < deadline:
                hdr = open(path, "rb").read(16)
                magic, seq, w, h = _st.unpack("<IIII", hdr)
                if magic == 0x48534648 and seq >= 2 and seq % 2 == 0:
                    break
                _t.sleep(0.05)
            assert seq >= 2

            s = _native.CaptureSettings()
            s.capture_width = 1280
            s.capture_height = 720
            s.capture_backend = f"shm:{path}"
            s.target_fps = 30
            s.output_mode = 1
            s.use_cpu = True
            s.gpu_id = -1
            s.video_fullframe = True
            s.video_crf = 12
            s.video_cbr_mode = False
            s.stripe_height = 720
            got = []
            done = threading.Event()

            def cb(data, frame_id, y, width, height, key, *a):
                got.append(bytes(data))
                done.set()

            cap = _native.ScreenCapture()
            cap.start_capture(cb, s)
            assert done.wait(8)
            cap.stop_capture()
            dy, _, _ = Decoder().decode(got[0][10:])[0]
            # the client's map_window fills its buffer with 0x42 bytes
            # (B=G=R=0x42 -> luma 0x42); decoded pixels must match
            assert abs(int(dy[5, 5]) - 0x42) <= 2
            assert abs(int(dy[350, 600]) - 0x42) <= 2
        finally:
            comp.stop_shm_publisher()
    finally:
        cli.close()
