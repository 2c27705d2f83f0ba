"""k_render_layers_grad mutant (profiles/render_layers_grad/mutants.txt): of two taps that replicate addressing puts on one
texel only one is added."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    '    atomicAdd(g + tp.i01, v * tp.w01);',
    '    if (tp.i01 != tp.i00) atomicAdd(g + tp.i01, v * tp.w01);')
sub(sys.argv[1], F,
    '    atomicAdd(g + tp.i10, v * tp.w10);',
    '    if (tp.i10 != tp.i00) atomicAdd(g + tp.i10, v * tp.w10);')
