"""k_render_layers_depth_grad mutant (profiles/render_depth_grad/mutants.txt): every layer's gz scaled by layer 0's
inv_texel."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip",
    'sums[(2 * lay) * kBlock] += (double)z.inv_texel[lay] * (Pv * sy - Pu * sx);',
    'sums[(2 * lay) * kBlock] += (double)z.inv_texel[0] * (Pv * sy - Pu * sx);')
