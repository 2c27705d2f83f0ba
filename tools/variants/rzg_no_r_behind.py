"""k_render_layers_depth_grad mutant (profiles/render_depth_grad/mutants.txt): R_{l+1} dropped from e_l, e_l = T_l D_l."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip",
    'const double el = Tl * d, gl = Tl * cover;',
    'const double el = Tl * D, gl = Tl * cover;')
