"""k_render_layers mutant (profiles/render_layers/mutants.txt): every layer is looked up with layer 0's inv_texel."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'const Taps taps(at.ox, at.oy, a.inv_texel[l], a.Ht, a.Wt);',
    'const Taps taps(at.ox, at.oy, a.inv_texel[0], a.Ht, a.Wt);')
