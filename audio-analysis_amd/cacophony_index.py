"""Drop-in for the reference's ``src/cacophony_index.py`` import surface
(``import cacophony_index; cacophony_index.calculate(file)``,
src/analyse.py:440-443)."""
from aa_amd.cacophony_index import (apply_correction_curve_202001C, calculate, points_device,  # noqa: F401
                                    score_from_points, score_table)
