"""k_render_layers_grad mutant (profiles/render_layers_grad/mutants.txt): the front-to-back walk stops where T reaches 0, as the
forward's does, also when a coverage gradient is asked for: the layers behind an opaque texel are not read, R starts there at 0."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip",
    'if (!b.galpha && Tm == 0.0) break;',
    'if (Tm == 0.0) break;')
