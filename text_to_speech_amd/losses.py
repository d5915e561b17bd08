"""The reference's TacotronLoss (custom_train_objects/losses/tacotron_loss.py) for evaluation: the per-sample values
`loss`, `<kind>_mel_loss`, `<kind>_mel_postnet_loss`, `gate_loss` of a teacher-forced batch, computed on the GPU by one
reduction pass (`HipEngine.tacotron2_loss`, tts_hip_tacotron2_loss).  No gradient: backward passes and optimizers are out of
scope.  The math is pinned in include/tts_hip.h and restated in float64 by tests/taco_loss_ref.py.
"""
from __future__ import annotations

import numpy as np

MEL_LOSS_KINDS = {'mse': 0, 'mae': 1, 'weighted_mse': 2, 'weighted_mae': 3}        # TTS_HIP_LOSS_*


def mel_loss_kinds(mel_loss):
    """`mel_loss` as the reference takes it (a name or a list / tuple of names) -> the list of names, checked: 1 to 4 distinct
    kinds of `MEL_LOSS_KINDS`, in the caller's order.  The reference's 'similarity' (it needs a model of its own) and callables
    are refused by name."""
    kinds = list(mel_loss) if isinstance(mel_loss, (list, tuple)) else [mel_loss]
    for kind in kinds:
        if callable(kind):
            raise ValueError(f'mel_loss: a callable ({getattr(kind, "__name__", kind)!r}) cannot run on the GPU; '
                             f'use one of {tuple(MEL_LOSS_KINDS)}')
        if kind == 'similarity':
            raise ValueError(f"mel_loss 'similarity' needs a similarity model and is not supported; use one of {tuple(MEL_LOSS_KINDS)}")
        if kind not in MEL_LOSS_KINDS:
            raise ValueError(f'unknown mel_loss {kind!r}; use one of {tuple(MEL_LOSS_KINDS)}')
    if not 1 <= len(kinds) <= len(MEL_LOSS_KINDS):
        raise ValueError(f'mel_loss must name 1 to {len(MEL_LOSS_KINDS)} kinds, got {len(kinds)}')
    if len(set(kinds)) != len(kinds):
        raise ValueError(f'mel_loss names a kind twice: {kinds}')
    return kinds


def loss_output_names(mel_loss):
    """The rows of a loss result, the reference's `TacotronLoss.output_names` (tacotron_loss.py:52-60)."""
    kinds = list(mel_loss) if isinstance(mel_loss, (list, tuple)) else [mel_loss]
    return (['loss'] + [f'{k}_mel_loss' for k in kinds] + [f'{k}_mel_postnet_loss' for k in kinds] + ['gate_loss'])


class TacotronLoss:
    """loss = gate_loss + every mel loss (on decoder_output) + every postnet mel loss (on mel), per sample.  Constructor
    arguments, `output_names` and `get_config()` are the reference's.  `label_smoothing` is kept in the config and, as in the
    reference's `call`, never applied; `similarity_function` is kept for the signature only (`mel_loss='similarity'` is
    refused).  Behaviour is specified for finite inputs only: the padding mask multiplies the error, so a non-finite value in
    a masked frame propagates, as it does in the reference."""

    def __init__(self, from_logits=False, label_smoothing=0, mel_loss='mse', mask_mel_padding=True, similarity_function=None,
                 finish_weight=1., not_finish_weight=1., name='tacotron_loss', reduction='sum_over_batch_size', **kwargs):
        if kwargs:
            raise TypeError(f'unexpected arguments {sorted(kwargs)}')
        mel_loss_kinds(mel_loss)
        self.name, self.reduction = name, reduction
        self.mask_mel_padding = mask_mel_padding
        self.label_smoothing = label_smoothing
        self.from_logits = from_logits
        self.finish_weight = finish_weight
        self.not_finish_weight = not_finish_weight
        self.mel_loss = mel_loss
        self.similarity_function = similarity_function

    @property
    def output_names(self):
        return loss_output_names(self.mel_loss)

    def __call__(self, y_true, y_pred, engine=None, stream=None):
        """y_true = [mel_target [B, T, 80], gate_target [B, T]], y_pred = [decoder_output, mel, stop_tokens, ...] (the first
        three entries are read: a Tacotron2ForwardOutput fits) -> float32 [K, B], rows as `output_names`, per sample (the
        reference's `reduction` over the batch is the caller's: `evaluate` reports the mean).  `engine`: the HipEngine (or a
        runtime with `tacotron2_loss`) to run on -- there is no host implementation."""
        if engine is None or not hasattr(engine, 'tacotron2_loss'):
            raise ValueError('TacotronLoss needs engine= (a HipEngine or HipRuntime): the loss runs on the GPU')
        mel_target, gate_target = y_true
        decoder_output, mel, stop_tokens = y_pred[:3]
        extra = {} if stream is None else {'stream': stream}
        return engine.tacotron2_loss(mel_target, gate_target, decoder_output, mel, stop_tokens, mel_loss=self.mel_loss,
                                     mask_mel_padding=self.mask_mel_padding, from_logits=self.from_logits,
                                     finish_weight=self.finish_weight, not_finish_weight=self.not_finish_weight, **extra)

    def get_config(self):
        mel_loss = list(self.mel_loss) if isinstance(self.mel_loss, (list, tuple)) else self.mel_loss
        return {'name': self.name, 'reduction': self.reduction, 'mask_mel_padding': self.mask_mel_padding,
                'label_smoothing': self.label_smoothing, 'finish_weight': self.finish_weight,
                'not_finish_weight': self.not_finish_weight, 'from_logits': self.from_logits, 'mel_loss': mel_loss}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


def mean_losses(names, per_item):
    """{name: the mean of its row of `per_item` [K, N] as a float}"""
    per_item = np.asarray(per_item, dtype=np.float64)
    return {name: float(per_item[k].mean()) for k, name in enumerate(names)}
