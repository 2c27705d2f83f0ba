"""k_render_layers_grad mutant (profiles/render_layers_grad/mutants.txt): the layer stride of gtex confused with the other
kind.  The confusion the issue names -- a SHARED gradient addressed with the per-layer stride -- writes past the end of the
shared buffer and is not run on a GPU; this is its in-bounds mirror image: a per-layer gradient addressed with stride 0, every
layer adding into layer 0's planes."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip",
    'double* __restrict__ gt = b.gtex + m * b.gtex_layer_stride;',
    'double* __restrict__ gt = b.gtex + m * (b.gtex_layer_stride ? 0 : b.gtex_layer_stride);')
