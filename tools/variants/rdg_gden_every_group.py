"""k_render_layers_dp_grad mutant (profiles/render_dp_grad/mutants.txt): gden counted in every group of four planes, not in the first only."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'e.gden = t0 == 0 ? gden : nullptr;',
    'e.gden = gden;')
