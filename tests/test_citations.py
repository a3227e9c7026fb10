"""Every `File.ext:line[-line]` citation of a reference file in the public header, the kernels' headers, the oracle and the
docs must point inside that file.  The reference files' line counts are stored in tests/golden/reference_line_counts.json
(tests/golden/make_reference_line_counts.py writes it from a reference tree)."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["include/dindel_hmm.h", "oracle/dd_oracle.c", "oracle/dd_oracle.h", "oracle/ref_bits.cpp", "DESIGN.md", "INTEGRATION.md",
         "dindel_tgi_amd/csrc/hmm_kernel.hip", "dindel_tgi_amd/csrc/faster_kernel.hip", "dindel_tgi_amd/csrc/genotype_kernel.hip",
         "dindel_tgi_amd/csrc/capi_internal.h", "dindel_tgi_amd/csrc/plan.cpp", "dindel_tgi_amd/csrc/batch_host.cpp",
         "dindel_tgi_amd/csrc/launch.cpp", "dindel_tgi_amd/csrc/host_path.cpp", "dindel_tgi_amd/host/compute_likelihoods.hpp", "dindel_tgi_amd/host/compute_likelihoods.cpp",
         "dindel_tgi_amd/host/genotype.hpp", "dindel_tgi_amd/host/genotype.cpp", "dindel_tgi_amd/host/cigar.hpp",
         "dindel_tgi_amd/host/cigar.cpp", "dindel_tgi_amd/host/dindel_types.hpp", "dindel_tgi_amd/host/glf_output.hpp",
         "dindel_tgi_amd/host/glf_to_vcf.hpp", "dindel_tgi_amd/host/glf_to_vcf.cpp", "dindel_tgi_amd/host/bam_reader.hpp",
         "dindel_tgi_amd/host/window_io.hpp", "dindel_tgi_amd/host/window_io.cpp", "dindel_tgi_amd/host/get_reads.hpp",
         "dindel_tgi_amd/host/get_reads.cpp", "dindel_tgi_amd/host/diploid_glf.hpp", "dindel_tgi_amd/host/diploid_glf.cpp",
         "dindel_tgi_amd/host/dindel_gpu.cpp", "dindel_tgi_amd/host/dindel_glf2vcf.cpp", "tests/_vcf_oracle.py", "profiles/r02/instruction_mix.md",
         "dindel_tgi_amd/host/realigned_bam.hpp", "dindel_tgi_amd/host/realigned_bam.cpp", "dindel_tgi_amd/host/bam_reader.cpp",
         "tests/_getreads_oracle.py", "profiles/r02/n2_pipeline.md", "tests/_param_cases.py", "tests/test_param_cases_cpu.py"]


def test_reference_citations_point_inside_the_files():
    nlines = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")))["nlines"]
    pat = re.compile(r"((?:python/)?[A-Za-z][A-Za-z0-9_]*\.(?:cpp|hpp|py|h))`?:(\d+)(?:-(\d+))?")
    bad, n = [], 0
    for rel in FILES:
        for m in pat.finditer(open(os.path.join(ROOT, rel)).read()):
            name, a, b = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            if name not in nlines:
                continue                                  # our own files (hmm_kernel.hip:…, plan.cpp …) are not reference citations
            n += 1
            if not (1 <= a <= b <= nlines[name]):
                bad.append((rel, m.group(0), nlines[name]))
    assert n > 150, n
    assert not bad, bad
