"""Drop-in for the parts of the reference's models/fastpitch/fastpitch package that have a device implementation of their own:
`alignment` (monotonic alignment search) and `model` (average_pitch, mask_from_lens).  The model itself is models.fastpitch.networks.FastPitch."""
