"""ppyolo_hip/hostio.py without a GPU: the staging ring's state machine, the host pool, the device rule, the in-place image
rule as one table run once per caller noun, and the staging buffer a refused `out=` used to leak in JpegDecoder.decode."""
import threading

import pytest
import torch

from ppyolo_hip import hostio
from ppyolo_hip._lib import PPYoloHipError


class Event(object):
    """What hostio.Staging expects of an event: recorded when made, synchronize() on the host."""
    log = []

    def __init__(self):
        Event.log.append(('record', id(self)))

    def synchronize(self):
        Event.log.append(('wait', id(self)))


# ---- the ring ---------------------------------------------------------------------------------------------------------------
def test_ring_state_machine():
    """tests/test_gpu_jpeg.py::test_host_batches_own_their_staging_buffer on StagingRing alone."""
    Event.log = []
    ring = hostio.StagingRing('cpu', 64, stage='entropy', event=Event)
    a = ring.take(10)
    b = ring.take(100)
    assert a[0] != b[0] and a[2].numel() == 64 and b[2].numel() == 100 and not a[2].is_pinned()
    with pytest.raises(PPYoloHipError, match='the entropy stage may run at most two batches ahead'):
        ring.take(10)
    with ring.uploading(*b[:2]) as st:                 # b reaches the device: its slot is free again
        assert st is ring.slots[b[0]] and st.buffer is b[2] and Event.log == []
    assert Event.log == [('record', id(st.busy))]
    c = ring.take(10)
    assert c[0] == b[0] and c[1] == b[1] + 1 and Event.log[-1] == ('wait', Event.log[0][1])      # take() waited for b's copy
    assert c[2] is b[2] and c[2].numel() == 100         # grown once, never shrunk
    ring.release(*c[:2])                                # a released batch frees its slot
    for _ in range(2):                                  # the same handle may bracket an upload twice: the second waits for the first copy
        before = len(Event.log)
        with ring.uploading(*a[:2]) as st:
            waited = Event.log[before:]
        assert waited == ([] if _ == 0 else [('wait', first)])
        first = id(st.busy)
    d = ring.take(10)
    e = ring.take(10)
    assert {d[0], e[0]} == {0, 1} and a[:2] not in (d[:2], e[:2]) and b[:2] not in (d[:2], e[:2]) and c[:2] not in (d[:2], e[:2])
    for old in (a, b, c):
        with pytest.raises(PPYoloHipError, match='stale HostBatch'):
            with ring.uploading(*old[:2]):
                pytest.fail('a stale batch was let in')
        ring.release(*old[:2])                          # releasing a stale handle is a no-op: d and e still hold both slots
    with pytest.raises(PPYoloHipError, match='two batches ahead'):
        ring.take(10)
    with pytest.raises(ZeroDivisionError):              # a failure inside the bracket: the batch never reached the device
        with ring.uploading(*d[:2]):
            1 / 0
    with pytest.raises(PPYoloHipError, match='two batches ahead'):
        ring.take(10)
    ring.release(*d[:2])
    assert ring.take(10)[0] == d[0]


def test_ring_take_and_upload_on_two_threads():
    ring = hostio.StagingRing('cpu', 16, event=Event)
    taken, errors = [], []

    def host():
        for _ in range(200):
            while True:
                try:
                    taken.append(ring.take(16)[:2])
                    break
                except PPYoloHipError:
                    pass

    t = threading.Thread(target=host)
    t.start()
    done = 0
    while done < 200:
        if done < len(taken):
            try:
                with ring.uploading(*taken[done]):
                    pass
            except PPYoloHipError as e:
                errors.append(e)
            done += 1
    t.join()
    assert not errors and len(set(taken)) == 200


def test_staging_grows_by_its_factor_and_has_no_event_on_the_cpu():
    st = hostio.Staging('cpu', 64, factor=2)
    assert st.acquire(10).numel() == 64 and st.acquire(100).numel() == 200 and st.acquire(150).numel() == 200
    st.buffer[:4] = torch.tensor([1, 2, 3, 4], dtype=torch.uint8)
    assert st.upload(4).tolist() == [1, 2, 3, 4] and st.busy is None
    Event.log = []
    st = hostio.Staging('cpu', 8, event=Event)
    st.acquire(8)
    st.upload(8)
    st.acquire(8)
    assert [k for k, _ in Event.log] == ['record', 'wait'] and st.busy is None


# ---- the pool ---------------------------------------------------------------------------------------------------------------
def test_host_pool():
    assert hostio.MAX_THREADS == 16 and hostio.HostPool(64, 'p').threads == 16 and hostio.HostPool(None, 'p').threads is None
    with pytest.raises(PPYoloHipError, match='threads must be >= 1'):
        hostio.HostPool(0, 'p')
    one = hostio.HostPool(1, 'p')
    assert one.map(lambda i: i * i, 5) == [0, 1, 4, 9, 16] and one.executor is None
    many = hostio.HostPool(None, 'ppy-test')
    assert many.map(lambda i: i, 1) == [0] and many.executor is None            # one item: no executor either
    names = many.map(lambda i: (i, threading.current_thread().name), 40)
    assert [i for i, _ in names] == list(range(40)) and all(n.startswith('ppy-test') for _, n in names)
    assert many.executor._max_workers == 16

    def boom(i):
        if i == 3:
            raise KeyError('worker 3')
        return i

    with pytest.raises(KeyError, match='worker 3'):
        many.map(boom, 8)


# ---- the device rule --------------------------------------------------------------------------------------------------------
def test_same_device_without_cuda(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('the CUDA runtime was asked'))
    cpu, cuda = torch.device('cpu'), torch.device('cuda')
    assert hostio.same_device(cpu, cpu) and hostio.same_device('cpu', torch.zeros(1).device)
    assert not hostio.same_device(cpu, cuda) and not hostio.same_device(cuda, cpu) and not hostio.same_device('meta', cpu)
    assert hostio.same_device(cuda, cuda) and hostio.same_device('cuda:1', 'cuda:1') and not hostio.same_device('cuda:0', 'cuda:1')


def test_same_device_resolves_a_missing_index_to_the_current_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 1)
    assert hostio.same_device('cuda', 'cuda:1') and hostio.same_device('cuda:1', 'cuda')
    assert not hostio.same_device('cuda', 'cuda:0') and not hostio.same_device('cuda:0', 'cuda')


# ---- the in-place image rule ------------------------------------------------------------------------------------------------
H, W = 6, 5
OK = torch.zeros((H, W, 3), dtype=torch.uint8)
BIG = torch.zeros((H + 7, W + 9, 3), dtype=torch.uint8)
GOOD = {'contiguous': OK, 'crop': BIG[3:3 + H, 5:5 + W], 'one row, row stride 0': OK[:1].expand(1, W, 3),
        'one row, row stride 1': torch.as_strided(OK, (1, W, 3), (1, 3, 1))}
BAD = [('float dtype', OK.float(), 'cpu', 'dtype torch.float32'),
       ('float dtype names uint8', OK.float(), 'cpu', 'uint8'),
       ('2-D', OK[:, :, 0], 'cpu', r'shape \(6, 5\)'),
       ('2-D is no uint8 image', OK[:, :, 0], 'cpu', 'uint8 image'),
       ('4 channels', torch.zeros((H, W, 4), dtype=torch.uint8), 'cpu', r'shape \(6, 5, 4\)'),
       ('4 channels sliced to 3', torch.zeros((H, W, 4), dtype=torch.uint8)[:, :, :3], 'cpu', 'strides.*pixel stride 3'),
       ('[:, ::2]', torch.zeros((H, 2 * W, 3), dtype=torch.uint8)[:, ::2], 'cpu', 'strides.*pixel stride 3'),
       ('permute(1, 0, 2)', torch.zeros((W, H, 3), dtype=torch.uint8).permute(1, 0, 2), 'cpu', 'strides'),
       ('CHW storage', torch.zeros((3, H, W), dtype=torch.uint8).permute(1, 2, 0), 'cpu', 'strides'),
       ('expand with row stride 0', OK[:1].expand(4, W, 3), 'cpu', 'strides'),
       ('0 rows', torch.zeros((0, W, 3), dtype=torch.uint8), 'cpu', '0, width and height must be'),
       ('wrong device', OK, 'cuda', 'lives on cpu'),
       ('another wrong device', torch.empty((H, W, 3), dtype=torch.uint8, device='meta'), 'cpu', 'lives on meta'),
       ('a Python list', [[1, 2, 3]], 'cpu', 'expected a uint8 tensor.*list')]


@pytest.mark.parametrize('noun,label', [('source', 'image 1'), ('output', 'output 1'), ('drawing in place', 'image 1')])
def test_image_rule(noun, label):
    for name, t in GOOD.items():
        assert hostio.check_image(1, t, 'cpu', noun) is t, name
        assert hostio.row_pitch(t) >= 3 * W and (t.shape[0] == 1 or hostio.row_pitch(t) == t.stride(0)), name
    for name, t, device, word in BAD:
        with pytest.raises(PPYoloHipError, match='^%s.*%s' % (label, word)):
            hostio.check_image(1, t, device, noun)
            pytest.fail(name)
    with pytest.raises(PPYoloHipError, match=r'^image: shape \(6, 5\)' if noun != 'output' else r'^output: shape'):
        hostio.check_image(None, OK[:, :, 0], 'cpu', noun)             # no index: augment.source_image
    # the encoder's variant: grey passes with pixel stride 1, both sides are bounded
    grey = torch.zeros((H, 2 * W), dtype=torch.uint8)
    assert hostio.check_image(0, grey, 'cpu', noun, grey=True) is grey
    with pytest.raises(PPYoloHipError, match='strides.*pixel stride 1 and rows'):
        hostio.check_image(0, grey[:, ::2], 'cpu', noun, grey=True)
    with pytest.raises(PPYoloHipError, match='strides'):
        hostio.check_image(0, OK[:, :, 0], 'cpu', noun, grey=True)     # one channel of a colour image: pixel stride 3
    for t in (torch.zeros((0, 4, 3), dtype=torch.uint8), torch.zeros((1, 65536), dtype=torch.uint8)):
        with pytest.raises(PPYoloHipError, match=r'1\.\.65535'):
            hostio.check_image(0, t, 'cpu', noun, grey=True, bound=True)
    assert hostio.check_image(0, torch.zeros((1, 65535), dtype=torch.uint8), 'cpu', noun, grey=True, bound=True) is not None
    # host memory, where the caller takes it by value: any strides, but dtype and shape still hold
    loose = torch.zeros((H, 2 * W, 3), dtype=torch.uint8)[:, ::2]
    assert hostio.check_image(0, loose, 'cuda', noun, host=True) is loose
    with pytest.raises(PPYoloHipError, match='dtype'):
        hostio.check_image(0, loose.float(), 'cuda', noun, host=True)


def test_check_outputs_wants_device_tensors_of_the_exact_shape():
    for bad in (OK, OK.float(), None):                                  # (nothing here is on a device: every case stops at the first rule)
        with pytest.raises(PPYoloHipError, match=r'output 0 must be a uint8 device tensor \[6, 5, 3\]'):
            hostio.check_outputs([bad, OK], [(H, W), (H, W)], 'cpu')
    with pytest.raises(PPYoloHipError, match='1 output tensors for 2 images'):
        hostio.check_outputs([OK], [(H, W), (H, W)], 'cpu')


def test_read_bytes(tmp_path):
    p = tmp_path / 'f.bin'
    p.write_bytes(b'abc')
    assert hostio.read_bytes(p) == hostio.read_bytes(str(p)) == hostio.read_bytes(memoryview(b'abc')) == hostio.read_bytes(bytearray(b'abc')) == b'abc'
    with pytest.raises(PPYoloHipError, match='got int'):
        hostio.read_bytes(3)


# ---- the leak ---------------------------------------------------------------------------------------------------------------
def test_a_refused_out_gives_the_jpeg_decoders_buffer_back():
    """JpegDecoder.decode used to leave the HostBatch held when reconstruct() refused `out=`: the third call then failed with
    'two batches ahead' instead of the refusal.  Needs the built library (host entropy stage), not a GPU."""
    import jpeg_entropy_util as U
    import jpeg_fixtures as F
    U.lib()
    from ppyolo_hip.jpeg import JpegDecoder
    d = JpegDecoder(device='cpu')
    h, w, _ = F.pixels('c420_5x5').shape
    for _ in range(3):
        with pytest.raises(PPYoloHipError, match=r'output 0 must be a uint8 device tensor \[%d, %d, 3\]' % (h, w)):
            d.decode([F.data('c420_5x5')], out=[torch.empty((h, w, 3), dtype=torch.uint8)])
    hb = d.entropy_decode([F.data('c420_5x5')])
    assert hb.n == 1 and hb.stage is d._ring.slots[hb.slot].buffer
    d.release(hb)
