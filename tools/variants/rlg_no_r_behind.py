"""k_render_layers_grad mutant (profiles/render_layers_grad/mutants.txt): R_{l+1} dropped from the coverage gradient, e_l = T_l D_l."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip",
    'scatter_taps(b.galpha + m * plane, tp, Tb * d);',
    'scatter_taps(b.galpha + m * plane, tp, Tb * D);')
