"""Mirror of the reference's rec/io package for the index streams the beam-search coder emits."""
from .entropy_coding import ArithmeticCoder  # noqa: F401
from .utils import write_compressed_code, read_compressed_code, encode_files, decode_files  # noqa: F401
from .utils import encode_files_device, decode_files_device, rec_header_words, rec_files_max_K, header_seed  # noqa: F401
from .utils import encode_files_ragged, decode_files_ragged, encode_files_device_ragged, decode_files_device_ragged  # noqa: F401
from .segmented import encode_files_segmented, decode_files_segmented, encode_files_device_segmented  # noqa: F401
from .segmented import decode_files_device_segmented, segment_blocks_of, segmented_header_words, is_segmented  # noqa: F401
from .tables import SymbolTables, RowHistograms, hist_rows, tables_from_histograms  # noqa: F401
from .residual import encode_residuals, decode_residuals, encode_residuals_device, decode_residuals_device  # noqa: F401
from .residual import residual_model_bits, res_status_text  # noqa: F401
from .residual import cost_table, scale_bits, scale_bits_device, residual_model_bits_device, fit_scales  # noqa: F401
