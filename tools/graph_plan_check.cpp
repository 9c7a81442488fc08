// Host soundness of the graph planner: plans node tables through aa_graph_plan
// and reads every node's plan, name and images back, in a plain program that
// is built with the host sanitizers (tools/graph_plan_check.py builds and runs
// it on the CPU; it never touches a GPU).
//
// argv: table files written by tools/graph_plan_check.py --
//   int32 n_nodes, in_h, in_w, in_c, precision, nofuse; int64 blob_len;
//   aa_node[n_nodes]; float[blob_len]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "aa.h"

static int plan_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return fprintf(stderr, "%s: cannot open\n", path), 1;
    int32_t h[6];
    int64_t blob_len = 0;
    if (fread(h, sizeof h, 1, f) != 1 || fread(&blob_len, sizeof blob_len, 1, f) != 1) return fclose(f), 1;
    std::vector<aa_node> nodes(h[0]);
    std::vector<float> blob(blob_len);  // exactly blob_len floats: a read past the blob is a heap overflow
    const bool ok = fread(nodes.data(), sizeof(aa_node), nodes.size(), f) == nodes.size() &&
                    fread(blob.data(), sizeof(float), blob.size(), f) == blob.size();
    fclose(f);
    if (!ok) return fprintf(stderr, "%s: short file\n", path), 1;
    if (h[5]) setenv("AA_GRAPH_NOFUSE", "1", 1);
    else unsetenv("AA_GRAPH_NOFUSE");
    void* g = nullptr;
    const int rc = aa_graph_plan(nodes.data(), h[0], blob.data(), blob_len, h[1], h[2], h[3], h[4], &g);
    if (rc != AA_OK) {
        printf("%s: refused (%d): %s\n", path, rc, aa_last_error());
        return 0;
    }
    aa_graph_layout lay;
    if (aa_graph_plan_layout(g, &lay) != AA_OK) return 1;
    size_t bytes = 0;
    const int n = aa_graph_n_stages(g);
    for (int i = 0; i < n; ++i) {
        aa_node_plan p;
        char name[96];
        double fl, by;
        if (aa_graph_node_plan(g, i, &p) != AA_OK || aa_graph_stage_info(g, i, name, sizeof name, &fl, &by) != AA_OK)
            return 1;
        for (int which = 0; which < 4; ++which) {
            size_t len = 0;
            if (aa_graph_node_image(g, i, which, nullptr, 0, &len) != AA_OK) return 1;
            std::vector<unsigned char> buf(len);
            if (aa_graph_node_image(g, i, which, buf.data(), len, &len) != AA_OK) return 1;
            bytes += len;
        }
    }
    printf("%s: %d nodes, %zu image bytes, workspace %zu B per window, %d outputs\n", path, n, bytes,
           aa_graph_workspace_bytes(g, 1), aa_graph_n_outputs(g));
    float x = 0.f;  // a plan refuses to run
    if (aa_graph_forward(g, &x, 1, &x, nullptr, &x, 4, nullptr) != AA_ERR_INVALID) return 1;
    return aa_graph_destroy(g) != AA_OK;
}

int main(int argc, char** argv) {
    void* g = nullptr;
    if (aa_graph_plan(nullptr, 0, nullptr, 0, 1, 1, 1, AA_PREC_BF16X3, &g) != AA_ERR_INVALID) return 1;
    for (int i = 1; i < argc; ++i)
        if (plan_file(argv[i])) return 1;
    printf("planned %d tables\n", argc - 1);
    return 0;
}
