"""include/USRP_buffer_generator.hpp with the sc16 surface of TX_buffer_generator: what the reference's server code would
include instead of its CUDA class must compile with plain g++ -std=c++11."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_generator_sc16_surface_compiles_with_gxx(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "USRP_buffer_generator.hpp"\n'
                   "int main(){ param p; p.buffer_len = 100; p.rate = 1000; p.decim = 0;\n"
                   " p.wave_type.push_back(TONES); p.freq.push_back(10); p.ampl.push_back(0.5f);\n"
                   " TX_buffer_generator gen(&p);\n"
                   " bool ok = gen.set_sc16_gain(16000.0f); float g = gen.sc16_gain();\n"
                   " gsdr_sc16* buf = nullptr; gen.get_sc16(&buf);\n"
                   " long long c = gen.sc16_clipped(); gen.close();\n"
                   " return ok && g > 0.f && c >= 0 && buf && sizeof(buf->i) == 2 ? 0 : 1; }\n")
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
