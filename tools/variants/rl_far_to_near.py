"""k_render_layers mutant (profiles/render_layers/mutants.txt): the layers are walked from the farthest to the nearest."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'for (int l = 0; l < a.L; ++l) {\n                const bool reads',
    'for (int l = a.L - 1; l >= 0; --l) {\n                const bool reads')
