"""k_render_layers mutant (profiles/render_layers/mutants.txt): the last layer does not update the transmittance, so the
coverage o = 1 - T is the one in front of the last layer (the colours are untouched: g is taken before the update)."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    '                T = T * (1.0 - al);\n            }',
    '                if (l + 1 < a.L) T = T * (1.0 - al);\n            }')
