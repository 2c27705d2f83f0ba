"""k_render_layers mutant (profiles/render_layers/mutants.txt): the ray is carried from layer to layer instead of from where the
trace left it to every layer."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'Ray at = r;\n                propagate_to<Ieee>(at, a.depth[l]);',
    'propagate_to<Ieee>(r, a.depth[l]);\n                Ray at = r;')
