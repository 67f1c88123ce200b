"""The tracker's host side without a device: Tracker's argument validation, and the refusals of ppy_track_update_f32 and the
sizes of ppy_track_state_bytes through the built library (every refusal comes before the launch; the pointers are never read)."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import _lib
    return _lib.lib()


def params(**kw):
    from ppyolo_hip import _lib
    v = dict(high_thresh=0.6, low_thresh=0.1, new_thresh=0.7, match_thresh=(0.2, 0.5, 0.3), max_lost=30, class_agnostic=0)
    v.update(kw)
    return _lib.TrackParams(v['high_thresh'], v['low_thresh'], v['new_thresh'], (ctypes.c_float * 3)(*v['match_thresh']), v['max_lost'],
                            v['class_agnostic'])


def call(lib, n=1, K=100, max_tracks=256, prm=None, state=16, state_bytes=None, dets=16, null_reason=False):
    """The entry point with pointers that are only compared with NULL -> (return code, reason)."""
    reason = ctypes.create_string_buffer(96)
    if state_bytes is None:
        state_bytes = n * (16 + 112 * max_tracks) if n > 0 and max_tracks > 0 else 0
    rc = lib.ppy_track_update_f32(dets, 16, n, K, max_tracks, ctypes.byref(prm) if prm is not None else None, state, state_bytes,
                                  16, 16, 16, 16, 16, None, 0, None if null_reason else reason, None)
    return rc, reason.value.decode()


def test_constants_mirror_the_header():
    import os
    import re
    from ppyolo_hip import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ppyolo_hip.h')).read()
    got = dict((k, int(v)) for k, v in re.findall(r'#define PPY_TRACK_(\w+) (\d+)', text))
    assert got == dict(FREE=_lib.TRACK_FREE, NEW=_lib.TRACK_NEW, TRACKED=_lib.TRACK_TRACKED, LOST=_lib.TRACK_LOST,
                       MAX_TRACKS=_lib.TRACK_MAX_TRACKS, MAX_ROWS=_lib.TRACK_MAX_ROWS)
    assert got['MAX_TRACKS'] >= 256 and ctypes.sizeof(_lib.TrackParams) == 32


def test_state_and_workspace_sizes(lib):
    import track_ref as R
    assert lib.ppy_track_state_bytes(1, 1) == 16 + 112 == 4 * (R.HEAD_WORDS + R.SLOT_WORDS)
    assert lib.ppy_track_state_bytes(3, 256) == 3 * (16 + 112 * 256)
    assert lib.ppy_track_state_bytes(2, 1024) == 2 * (16 + 112 * 1024)
    for n, t in ((0, 256), (1, 0), (1, 1025), (-1, 4)):
        assert lib.ppy_track_state_bytes(n, t) == 0
    assert lib.ppy_track_workspace_bytes(8, 1024, 1024) == 0


@pytest.mark.parametrize('kw,word', [
    (dict(max_tracks=0), 'max_tracks = 0, supported: 1..1024'), (dict(max_tracks=1025), 'max_tracks = 1025, supported: 1..1024'),
    (dict(K=0), 'K = 0 rows per frame, supported: 1..1024'), (dict(K=1025), 'K = 1025 rows per frame'),
    (dict(high_thresh=float('nan')), 'high_thresh is NaN'), (dict(low_thresh=float('nan')), 'low_thresh is NaN'),
    (dict(new_thresh=float('nan')), 'new_thresh is NaN'), (dict(match_thresh=(0.2, float('nan'), 0.3)), r'match_thresh\[1\] is NaN'),
    (dict(match_thresh=(0.2, 0.5, float('nan'))), r'match_thresh\[2\] is NaN'), (dict(max_lost=-1), 'max_lost = -1, must be at least 0')])
def test_limits_are_refused_by_name(lib, kw, word):
    import re
    shape = dict((k, kw.pop(k)) for k in ('max_tracks', 'K') if k in kw)
    rc, reason = call(lib, prm=params(**kw), **shape)
    assert rc == -2 and re.search(word, reason), (rc, reason)
    assert call(lib, prm=params(**kw), null_reason=True, **shape)[0] == -2          # h_reason may be NULL


def test_bad_arguments(lib):
    ok = params()
    assert call(lib, prm=None) == (-1, '')
    assert call(lib, prm=ok, n=0) == (-1, '')
    assert call(lib, prm=ok, n=65536) == (-1, '')
    assert call(lib, prm=ok, dets=None) == (-1, '')
    assert call(lib, prm=ok, state=None) == (-1, '')
    assert call(lib, prm=ok, state=24) == (-1, '')                                   # not 16-byte aligned
    assert call(lib, prm=ok, state_bytes=16 + 112 * 256 - 1) == (-1, '')             # one byte short
    assert call(lib, prm=ok, n=2, state_bytes=16 + 112 * 256) == (-1, '')            # the state of one stream for two


@pytest.mark.parametrize('kw,word', [
    (dict(streams=0), 'streams = 0, supported: 1..65535'), (dict(streams=65536), 'streams = 65536'),
    (dict(max_tracks=0), 'max_tracks = 0, supported: 1..1024'), (dict(max_tracks=1025), 'max_tracks = 1025'),
    (dict(max_lost=-1), 'max_lost = -1'), (dict(high_thresh=float('nan')), 'high_thresh is NaN'),
    (dict(low_thresh=float('nan')), 'low_thresh is NaN'), (dict(new_thresh=float('nan')), 'new_thresh is NaN'),
    (dict(match_thresh=(0.2, float('nan'), 0.3)), r'match_thresh\[1\] is NaN'), (dict(match_thresh=(0.2, 0.5)), r'match_thresh=\(0.2, 0.5\)'),
    (dict(match_thresh=0.5), 'match_thresh=0.5'), (dict(high_thresh='high'), "high_thresh='high'"), (dict(max_tracks='many'), "max_tracks='many'")])
def test_tracker_validates_on_the_host(kw, word):
    """Every message names the value, and comes before anything touches a device."""
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.track import Tracker
    kw = dict(kw)
    streams = kw.pop('streams', 1)
    with pytest.raises(PPYoloHipError, match=word):
        Tracker(streams, 'cuda', **kw)


def test_new_thresh_defaults_to_high_plus_a_tenth(monkeypatch):
    import torch
    from ppyolo_hip import ops, track
    monkeypatch.setattr(ops, 'track_state', lambda n, t, device: torch.zeros(n * (16 + 112 * t), dtype=torch.uint8))
    t = track.Tracker(2, 'cpu', max_tracks=3, high_thresh=0.5)
    assert t.params.new_thresh == ctypes.c_float(0.5 + 0.1).value and t.params.high_thresh == 0.5 and t.params.class_agnostic == 0
    assert list(t.params.match_thresh) == [ctypes.c_float(v).value for v in (0.2, 0.5, 0.3)] and t.params.max_lost == 30
    assert track.Tracker(1, 'cpu', new_thresh=0.9, class_agnostic=True).params.new_thresh == ctypes.c_float(0.9).value
    assert t.state().shape == (2, 4 + 28 * 3) and not t.state().any()
