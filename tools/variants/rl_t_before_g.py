"""k_render_layers mutant (profiles/render_layers/mutants.txt): the transmittance is updated BEFORE the layer's share g is taken."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'const double g = T * al;',
    'T = T * (1.0 - al);\n                const double g = T * al;')
sub(sys.argv[1], F,
    '                T = T * (1.0 - al);\n            }',
    '            }')
