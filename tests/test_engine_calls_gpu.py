"""GPU: the three ways into every `HipEngine` call that accepts CUDA tensors give the same bits -- host arrays, CUDA tensors
with stream=None, and (where the call takes `stream`) CUDA tensors on a fresh torch.cuda.Stream.  The same kernels run on
staged copies of the same bytes, so the comparison is bitwise.  tests/test_engine_calls.py pins the library side of the host
route; this pins what it cannot see, torch's side of `HipEngine._call`.

The CUDA inputs are awkward on purpose: float64 (int64 for tokens) and a strided view, so every one of them is converted
into a temporary that nothing references once the call has returned.  On the stream route the default stream then
allocates poison of the same sizes and a large block at once and fills them with NaN while the engine's work may still be
running: were a temporary not marked as used on the caller's stream, the caching allocator would hand its block out again and
the result would differ from the host route.

Shapes are the smallest that still take each path: B = 2, T = 4 ragged [4, 2] (WaveGlow), Tin = 5 / max_len 8 / teacher-forced
T = 6 (Tacotron2), N = 3000 with lengths [3000, 1500], one mel plan of filter_length 1024, 8 frames and 2 iterations of
Griffin-Lim, rows of 1024 with counts [1024, 10].
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, T, TIN, MAX_LEN, TF, N, F, BINS = 2, 4, 5, 8, 6, 3000, 8, 513
LENS = [N, N // 2]
CFG = dict(sampling_rate=22050, n_mel_channels=80, filter_length=1024, hop_length=256, win_length=1024, mel_fmin=0.0,
           mel_fmax=8000.0)
KEYS, OFFS = [0x6d386fd6ef20a096, 7], [5, (1 << 32) - 2]


def _inputs():
    rng = np.random.default_rng(20)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    audio = rng.uniform(-0.5, 0.5, (B, N)) * (np.sin(np.arange(N) / 150.0) > 0)        # bursts between stretches of silence
    tokens = rng.integers(1, 148, (B, TIN)).astype(np.int32)
    tokens[1, 3:] = 0
    return dict(
        mel=f32(rng.uniform(-11.5, 1.2, (B, T, 80))), z=f32(rng.standard_normal((B, T * 32, 8))),
        wav=f32(rng.uniform(-0.5, 0.5, (B, T * 256))), tokens=tokens,
        masks=f32(rng.integers(0, 2, (B, MAX_LEN, 2, 256)) * 2), tf_masks=f32(rng.integers(0, 2, (B, TF, 2, 256)) * 2),
        frames=f32(rng.uniform(-4, 1, (B, TF, 80))), target=f32(rng.uniform(-4, 1, (B, TF, 80))),
        gate=f32(rng.integers(0, 2, (B, TF))), stop=f32(rng.uniform(0.05, 0.95, (B, TF))),
        audio=f32(audio), row=f32(audio[0]), noise=f32(rng.uniform(-0.01, 0.01, (B, 400))),
        spec=f32(np.abs(rng.standard_normal((B, F, BINS)))), phase=f32(rng.uniform(-3, 3, (B, F, BINS))),
        init=f32(rng.standard_normal((B, F, BINS, 2))), log_mel=f32(rng.uniform(-6, 0, (B, F, 80))),
        bias=f32(rng.uniform(0, 0.05, (BINS,))))


X = _inputs()


class Device:
    """numpy array -> an awkward CUDA tensor of the same values (float64 / int64, every other element of a wider buffer), and
    the poison that follows a stream call."""

    def __init__(self):
        self.sizes = []

    def __call__(self, a):
        import torch
        wide = torch.int64 if a.dtype.kind in 'iu' else torch.float64
        buf = torch.zeros((*a.shape[:-1], 2 * a.shape[-1]), dtype=wide, device='cuda')
        view = buf[..., ::2]
        view.copy_(torch.as_tensor(a))
        assert not view.is_contiguous() or a.shape[-1] == 1
        self.sizes.append(a.size)
        return view

    def poison(self):
        import torch
        junk = [torch.full((n,), float('nan'), dtype=torch.float32, device='cuda') for n in self.sizes for _ in range(2)]
        junk.append(torch.full((16 << 20,), float('nan'), dtype=torch.float32, device='cuda'))      # 64 MiB
        return junk


def _flat(result):
    """The arrays of a result (tensor, array, scalar, None or a tuple of those) as numpy arrays."""
    if result is None:
        return []
    if isinstance(result, (tuple, list)):
        return [a for r in result for a in _flat(r)]
    return [result.cpu().numpy() if hasattr(result, 'cpu') else np.asarray(result)]


def _routes(call, streamed):
    """`call(convert, kwargs)` on host arrays, on CUDA tensors, and on a fresh stream with poison behind it -> bitwise equal."""
    import torch
    host = _flat(call(lambda a: a, {}))
    assert host and all(isinstance(a, np.ndarray) for a in host)
    results = {'device': call(Device(), {})}
    if streamed:
        dev, st = Device(), torch.cuda.Stream()
        on_stream = call(dev, {'stream': st})
        junk = dev.poison()
        st.synchronize()
        results['stream'] = on_stream
        del junk
    for route, result in results.items():
        assert all(hasattr(r, 'is_cuda') and r.is_cuda for r in _leaves(result)), f'{route} route: not every output is a CUDA tensor'
        got = _flat(result)
        assert len(got) == len(host), route
        for i, (g, h) in enumerate(zip(got, host)):
            assert g.dtype == h.dtype and g.shape == h.shape and g.tobytes() == h.tobytes(), \
                f'{route} route, output {i}: differs from the host route'
    return host


def _leaves(result):
    if result is None:
        return []
    if isinstance(result, (tuple, list)):
        return [a for r in result for a in _leaves(r)]
    return [result]


def _decode(e, c, kw, **how):
    enc = e.tacotron2_encode(c(X['tokens']), **kw)
    try:
        return e.tacotron2_decode(enc, max_len=MAX_LEN, early_stopping=False, **how, **kw)
    finally:
        enc.close()


def _reencode(e, c, kw):
    enc = e.tacotron2_encode(c(X['tokens'][:, :3]), **kw)
    try:
        assert e.tacotron2_encode(c(X['tokens']), into=enc, **kw) is enc
        return e.tacotron2_forward(enc, c(X['frames']), [TF, 3], prenet_masks=c(X['tf_masks']), **kw)
    finally:
        enc.close()


def _loss_mixed(e, c, kw):
    """Any CUDA input makes a device call: here only two of the five are."""
    xs = [X['target'], X['gate'], X['frames'], X['target'][::-1].copy(), X['stop']]
    if isinstance(c, Device):
        xs[2], xs[4] = c(xs[2]), c(xs[4])
    return e.tacotron2_loss(*xs, mel_loss=['mse', 'weighted_mae'], **kw)


def _denoise_out(e, c, kw):
    """`out=` exists for CUDA input only: the tensor handed in comes back, holding what the host call returns."""
    if not isinstance(c, Device):
        return e.denoise(e.mel_fn(CFG), X['audio'], X['bias'], lengths=LENS)
    import torch
    out = torch.full((B, N), float('nan'), device='cuda')
    assert e.denoise(e.mel_fn(CFG), c(X['audio']), X['bias'], lengths=LENS, out=out, **kw) is out
    return out


# name -> (call(engine, convert, kwargs), takes `stream`)
CASES = {
    'waveglow_z': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), z=c(X['z']), **kw), True),
    'waveglow_zeros': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), **kw), True),
    'waveglow_ragged': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), z=c(X['z']), lengths=[4, 2], **kw), True),
    'waveglow_packed': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), z=c(X['z']), lengths=[4, 2], packed=True, **kw), True),
    'waveglow_seed': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), seed=11, offset=3, **kw), True),
    'waveglow_seed_ragged': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), seed=11, lengths=[4, 2], **kw), True),
    'waveglow_row_seeds': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), row_seeds=(KEYS, OFFS), **kw), True),
    'waveglow_row_seeds_packed': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), row_seeds=(KEYS, OFFS), lengths=[4, 2], packed=True,
                                                                    **kw), True),
    'waveglow_f16x3': (lambda e, c, kw: e.waveglow_infer(c(X['mel']), z=c(X['z']), precision='f16x3', **kw), True),
    'waveglow_encode': (lambda e, c, kw: e.waveglow_encode(c(X['wav']), c(X['mel']), **kw), True),
    'waveglow_encode_ragged': (lambda e, c, kw: e.waveglow_encode(c(X['wav']), c(X['mel']), lengths=[4, 2], **kw), True),
    'tacotron2_infer': (lambda e, c, kw: e.tacotron2_infer(c(X['tokens']), max_len=MAX_LEN, early_stopping=False,
                                                           prenet_masks=c(X['masks'])), False),
    'tacotron2_infer_row_mask_seeds': (lambda e, c, kw: e.tacotron2_infer(c(X['tokens']), max_len=MAX_LEN, early_stopping=False,
                                                                          row_mask_seeds=(KEYS, OFFS), want_attention=False), False),
    'tacotron2_decode': (lambda e, c, kw: _decode(e, c, kw), True),
    'tacotron2_decode_masks': (lambda e, c, kw: _decode(e, c, kw, prenet_masks=c(X['masks'])), True),
    'tacotron2_decode_mask_seed': (lambda e, c, kw: _decode(e, c, kw, mask_seed=(9, 2)), True),
    'tacotron2_decode_row_mask_seeds': (lambda e, c, kw: _decode(e, c, kw, row_mask_seeds=(KEYS, OFFS)), True),
    'tacotron2_forward': (lambda e, c, kw: e.tacotron2_forward(c(X['tokens']), c(X['frames']), **kw), True),
    'tacotron2_forward_masks': (lambda e, c, kw: e.tacotron2_forward(c(X['tokens']), c(X['frames']), [TF, 3],
                                                                     prenet_masks=c(X['tf_masks']), **kw), True),
    'tacotron2_forward_seed': (lambda e, c, kw: e.tacotron2_forward(c(X['tokens']), c(X['frames']), [TF, 3], seed=4, offset=1, **kw),
                               True),
    'tacotron2_forward_reencoded': (_reencode, True),
    'tacotron2_loss': (lambda e, c, kw: e.tacotron2_loss(c(X['target']), c(X['gate']), c(X['frames']), c(X['target'][::-1].copy()),
                                                         c(X['stop']), **kw), True),
    'tacotron2_loss_mixed': (_loss_mixed, True),
    'mel_stft': (lambda e, c, kw: e.mel_stft(c(X['audio']), **kw), True),
    'mel_stft_short_row': (lambda e, c, kw: e.mel_stft(c(X['row'][:700]), **kw), True),
    'mel_fn_run': (lambda e, c, kw: e.mel_fn_run(e.mel_fn(CFG), c(X['audio']), lengths=LENS, **kw), True),
    'stft_transform': (lambda e, c, kw: e.stft_transform(e.mel_fn(CFG), c(X['audio']), lengths=LENS), False),
    'stft_inverse': (lambda e, c, kw: e.stft_inverse(e.mel_fn(CFG), c(X['spec']), c(X['phase']), frames=[F, 3]), False),
    'griffin_lim': (lambda e, c, kw: e.griffin_lim(e.mel_fn(CFG), c(X['spec']), frames=[F, 4], n_iters=2, init=X['init'], **kw), True),
    'griffin_lim_log_mel': (lambda e, c, kw: e.griffin_lim(e.mel_fn(CFG), c(X['log_mel']), kind='log_mel', n_iters=2, **kw), True),
    'denoise': (lambda e, c, kw: e.denoise(e.mel_fn(CFG), c(X['audio']), X['bias'], strength=0.3, **kw), True),
    'denoise_out': (_denoise_out, True),
    'reduce_noise': (lambda e, c, kw: e.reduce_noise(c(X['audio']), lengths=LENS, noise_length=400, **kw), True),
    'reduce_noise_clip': (lambda e, c, kw: e.reduce_noise(c(X['audio']), noise=X['noise'], renormalize=True, **kw), True),
    'reduce_noise_row': (lambda e, c, kw: e.reduce_noise(c(X['row']), noise_length=300, **kw), True),
    'trim_silence': (lambda e, c, kw: e.trim_silence(c(X['audio']), rate=22050, lengths=LENS, window_length=0.01), False),
    'trim_silence_row': (lambda e, c, kw: e.trim_silence(c(X['row']), window_length=200, mode='end'), False),
    'resample': (lambda e, c, kw: e.resample(c(X['audio']), 22050, 16000, lengths=LENS, **kw), True),
    'resample_row': (lambda e, c, kw: e.resample(c(X['row']), 22050, 16000, **kw), True),
    'remove_silence': (lambda e, c, kw: e.remove_silence(c(X['audio']), 22050, lengths=LENS, **kw), True),
    'remove_silence_threshold': (lambda e, c, kw: e.remove_silence(c(X['audio']), 22050, method='threshold', mode='end', **kw), True),
}
# trim_silence returns host integers for a CUDA tensor too, and a 1-D host row of remove_silence comes back cut to its length
HOST_RESULTS = {'trim_silence', 'trim_silence_row'}


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_device_and_stream_routes_agree(gpu_engine, name):
    call, streamed = CASES[name]
    if name in HOST_RESULTS:
        host = _flat(call(gpu_engine, lambda a: a, {}))
        dev = _flat(call(gpu_engine, Device(), {}))
        assert len(host) == len(dev) == 2 and all(np.array_equal(h, d) and h.dtype == d.dtype for h, d in zip(host, dev))
        return
    host = _routes(lambda c, kw: call(gpu_engine, c, kw), streamed)
    assert all(np.isfinite(a).all() for a in host if a.dtype.kind == 'f'), 'the host route itself returned non-finite values'


@pytest.mark.parametrize('kind', ['normal', 'masks'])
def test_random_fills_on_a_stream_equal_the_synchronous_ones(gpu_engine, kind):
    """No host route exists: the synchronous call (the engine's own stream, then `synchronize`) against a caller's stream."""
    import torch
    draw = (lambda **kw: gpu_engine.random_normal((3, 1000), 21, offset=4, **kw)) if kind == 'normal' else \
        (lambda **kw: gpu_engine.random_prenet_masks(B, MAX_LEN, 21, offset=4, **kw))
    want = draw().cpu().numpy()
    st = torch.cuda.Stream()
    got = draw(stream=st)
    junk = torch.full((16 << 20,), float('nan'), device='cuda')
    st.synchronize()
    assert got.is_cuda and got.cpu().numpy().tobytes() == want.tobytes()
    assert np.isfinite(want).all() and (kind == 'normal' or set(np.unique(want)) == {0.0, 2.0})
    del junk


@pytest.mark.parametrize('with_out', [False, True])
@pytest.mark.parametrize('kind', ['normal', 'masks'])
def test_random_rows_on_a_stream_equal_the_synchronous_ones(gpu_engine, kind, with_out):
    """row_stride 1024, counts [1024, 10]: elements behind a row's count keep what `out=` held, or the zeros of a fresh tensor."""
    import torch
    rows = gpu_engine.random_normal_rows if kind == 'normal' else gpu_engine.random_prenet_masks_rows
    flat = (lambda n, b: gpu_engine.random_normal((n,), KEYS[b], OFFS[b])) if kind == 'normal' else \
        (lambda n, b: gpu_engine.random_prenet_masks_rows(n, [KEYS[b]], [OFFS[b]])[0])
    counts, rest = [1024, 10], 7.0 if with_out else 0.0
    outs = []
    for st in (None, torch.cuda.Stream()):
        out = torch.full((2, 1024), rest, device='cuda') if with_out else None
        got = rows(1024, KEYS, OFFS, counts=counts, stream=st, out=out)
        if st is not None:
            junk = torch.full((16 << 20,), float('nan'), device='cuda')
            st.synchronize()
            del junk
        assert got.is_cuda and tuple(got.shape) == (2, 1024) and (out is None or got is out)
        outs.append(got.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    for b, n in enumerate(counts):
        assert outs[0][b, :n].tobytes() == flat(n, b).cpu().numpy().tobytes(), b
        assert (outs[0][b, n:] == rest).all(), b
