"""What tests/test_gpu_nonfinite.py plants, and the two lists of rows that are excused from a rule of DESIGN.md, "Non-finite
values" - each entry with its reason.  tests/test_nonfinite_table.py holds the lists to the kernels: an excused row that in fact
keeps the rule fails there, and so does an excuse of a kind the contract does not allow.

The rows are those of tests/layout_table.py and of the three layer modules (decoder, encoder, dilated convolution), at their
shapes: the smallest that reach each dispatch."""
import layout_table as L
import test_gpu_decoder_layouts as DEC
import test_gpu_dilated_conv_layouts as CONV
import test_gpu_encoder_layouts as ENC

ROWS = list(L.ROWS) + DEC.ROWS + ENC.ROWS + CONV.ROWS
BY_NAME = {row.name: row for row in ROWS}
assert len(BY_NAME) == len(ROWS)

VALUES = {'nan': float('nan'), '+inf': float('inf'), '-inf': float('-inf')}

# Where the value goes when the middle of the last batch row is a place the output does not depend on.
# (row, argument) -> index into the argument WITHOUT its batch axis, or a function of the row's clean values (a list of arrays in
# the order of the arguments) that gives it: a lookup reads the two points its phase names and no other.
PLANT = {
    ('nn.get_note_moments', 'x'): (1, 2),            # a frame the mask gives to a note
    ('nn.pool_over_notes', 'x'): (1, 2),
    # window_size 8 of 16 taps: the middle of the response is cropped away, tap 1 is kept
    ('core.apply_window_to_impulse_response', 'impulse_response'): (L.T // 2, 1),
    # the point sample 160 reads: floor(phase 64)
    ('core.linear_lookup', 'wavetables'): lambda v: (160, int(float(v[0][L.B - 1, 160, 0]) * 64.0)),
    # the sample output 200 reads as its first point: 200 - floor(phase 64)
    ('core.variable_length_delay', 'audio'): lambda v: (200 - int(float(v[0][L.B - 1, 200, 0]) * 64.0),),
}


def plant_index(row, arg, values=None):
  """The element of the last batch row (of row 0 where the batch axis is 1, or where there is none) that takes the value."""
  batched = len(arg.shape) > 1 and arg.shape[0] in (1, L.B)
  rest = arg.shape[1:] if batched else arg.shape
  inner = PLANT.get((row.name, arg.name), tuple(s // 2 for s in rest))
  if callable(inner):
    inner = inner(values)
  assert len(inner) == len(rest) and all(0 <= i < s for i, s in zip(inner, rest)), (row.name, arg.name, inner)
  return ((arg.shape[0] - 1,) + inner) if batched else inner


def per_row(row, arg):
  """The argument has one row per batch row (and so a row 0 that the value was not put into)."""
  return len(arg.shape) > 1 and arg.shape[0] == L.B


# ---- R2: rows whose batch row 0 does NOT stay bit-equal when batch row 1 holds a non-finite value ------------------------------
# Outputs that reduce over the batch (Row.scalar) are not per-row and need no entry.  What may stand here: the Reverb family,
# whose kernel transforms batch rows in pairs, so that row 0 and row 1 share one complex FFT.
PAIRED_ROWS = 'rows are transformed two at a time as the real and imaginary part of one complex FFT: a NaN in one fills the other'
EXEMPT_ROWS = {
    'Reverb/one_ir': PAIRED_ROWS + ' (csrc/reverb.hip, one impulse response for the batch; with one per row each row has its own transform)',
}

# ---- R3, weak form: (row, argument) whose NaN the reference itself discards, so the outputs stay finite ------------------------
# The value names the line of the reference (ddsp/...) or of the fp64 truth that drops the element.
KEEPS_FINITE = {
    ('core.nan_to_num', 'x'): 'ddsp/core.py:202-204 nan_to_num: tf.where(is_nan(x), value, x) is the operation itself',
    ('nn.get_note_mask', 'q_pitch'): 'ddsp/training/nn.py get_note_mask: the mask is one_hot of a count of pitch CHANGES (q[t] != q[t - 1]), 0 or 1',
    ('HmmTranscriber.predict_midi', 'pitches'): 'ddsp/losses.py HmmTranscriber.predict_midi: the output is the Viterbi state path, whole numbers 0 .. n_pitches - 1',
    ('HmmTranscriber.predict_midi', 'amps'): 'ddsp/losses.py HmmTranscriber.predict_midi: the output is the Viterbi state path, whole numbers 0 .. n_pitches - 1',
    ('TWMLoss.predict_f0', 'f0_candidates'): 'ddsp/losses.py:940 TWMLoss.predict_f0: np.nanargmin over the candidates, then a gather - a candidate whose loss is a NaN is never the one taken',
    ('MfccTimeDistributedRnnEncoder', 'f0_scaled'): 'ddsp/training/encoders.py:40-44 ZEncoder.call: f0_scaled is an input "to get n_timesteps dynamically" - its shape is read, its values are not',
}
