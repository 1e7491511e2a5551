from .synthetic import SyntheticTextVideoLoader, synth_batch, synth_batch_v1  # noqa: F401
from .transforms import CaptionCache, pil_bilinear_coeffs, pil_nearest_table, resize_sizes, resize_tables  # noqa: F401
from .v1_input import U8VideoTransform, collate_u8  # noqa: F401
from .v2_input import collate_u8_v2, failed_clip  # noqa: F401
