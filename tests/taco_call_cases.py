"""The refusals of the Tacotron2 calls (csrc/taco_call.h), one row per reason, shared by the CPU test of the two checks
(tests/test_taco_call.py: csrc/host_check.cpp --taco-call under ASan / UBSan) and the GPU test of the real symbols
(tests/test_taco_call_gpu.py).  The good call both start from: B = 3 rows of Tin = 12 tokens, max_len = T = 33, a 512-wide
model, host memory."""
EINVAL, ENOTREADY = -1, -2
B, TIN, LEN = 3, 12, 33

BAD_TOKENS = 'bad argument (tokens is NULL, or B = {B} outside [1, 1024], or Tin = {Tin} outside [1, 4096])'
PRECISION = 'precision must be 0 (f32) or 1 (f16 weights), got {}'
NOT_READY = 'tacotron2 weights not finalized'
OTHER_WEIGHTS = 'encoded batch belongs to other weights (width 768, model 512)'

# (kind, reason, what is wrong: settings of --taco-call over the good call (`lens`: the mel_lengths), status, message behind "<who>: ")
REFUSALS = [
    ('encode', 'mem kind', dict(mem=7), EINVAL, 'bad mem kind 7'),
    ('encode', 'not ready', dict(ready=0), ENOTREADY, NOT_READY),
    ('encode', 'tokens NULL', dict(null='tokens'), EINVAL, BAD_TOKENS.format(B=B, Tin=TIN)),
    ('encode', 'B = 0', dict(B=0), EINVAL, BAD_TOKENS.format(B=0, Tin=TIN)),
    ('encode', 'B = 1025', dict(B=1025), EINVAL, BAD_TOKENS.format(B=1025, Tin=TIN)),
    ('encode', 'Tin = 0', dict(Tin=0), EINVAL, BAD_TOKENS.format(B=B, Tin=0)),
    ('encode', 'Tin = 4097', dict(Tin=4097), EINVAL, BAD_TOKENS.format(B=B, Tin=4097)),
    ('encode', 'speaker NULL', dict(spk_dim=256, null='speaker'), EINVAL, 'this model needs a speaker embedding'),
    ('decode', 'precision', dict(precision=2), EINVAL, PRECISION.format(2)),
    ('decode', 'mem kind', dict(mem=7), EINVAL, 'bad mem kind 7'),
    ('decode', 'not ready', dict(ready=0), ENOTREADY, NOT_READY),
    ('decode', 'encoded NULL', dict(null='encoded'), EINVAL, 'bad argument: encoded batch is NULL or empty'),
    ('decode', 'other weights', dict(enc=768), EINVAL, OTHER_WEIGHTS),
    ('decode', 'keys NULL', dict(masks=3, null='keys'), EINVAL, 'keys / offsets is NULL'),
    ('decode', 'offsets NULL', dict(masks=3, null='offsets'), EINVAL, 'keys / offsets is NULL'),
    ('decode', 'max_len = 0', dict(max_len=0), EINVAL, 'bad argument: max_len = 0 must be at least 1'),
    ('forward', 'precision', dict(precision=-1), EINVAL, PRECISION.format(-1)),
    ('forward', 'mem kind', dict(mem=7), EINVAL, 'bad mem kind 7'),
    ('forward', 'not ready', dict(ready=0), ENOTREADY, NOT_READY),
    ('forward', 'encoded NULL', dict(null='encoded'), EINVAL, 'encoded batch is NULL or empty'),
    ('forward', 'other weights', dict(enc=768), EINVAL, OTHER_WEIGHTS),
    ('forward', 'mel_input NULL', dict(null='mel'), EINVAL, 'mel_input or mel_lengths is NULL'),
    ('forward', 'mel_lengths NULL', dict(null='lens'), EINVAL, 'mel_input or mel_lengths is NULL'),
    ('forward', 'T = 0', dict(T=0), EINVAL, 'T = 0 must be at least 1'),
    ('forward', 'B * T above 65536', dict(T=21846), EINVAL, 'B*T too large (B = 3, T = 21846: above 65536 frames); split the batch'),
    ('forward', 'mel_lengths[1] = 0', dict(lens=(33, 0, 33)), EINVAL, 'mel_lengths[1] = 0 is outside [1, T = 33]'),
    ('forward', 'mel_lengths[2] = 34', dict(lens=(33, 1, 34)), EINVAL, 'mel_lengths[2] = 34 is outside [1, T = 33]'),
]
