/* A caller WITHOUT Python encodes prompts: load a text-tower model file written by coma_amd (HipCLIPTextModel.save -> sd_model_save),
 * read int32 token ids [S, 77] from a raw file (S = the capacity the model was recorded at), run sd_text_encode and write the fp16
 * embeddings [S, 77, 768] -- the UNet context sd_unet_set_context takes.  Built and run by tests/test_sd_text_gpu.py:
 *     gcc tests/c/run_text.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Lcoma_amd -lcoma_hip -L/opt/rocm/lib -lamdhip64 \
 *         -Wl,-rpath,$PWD/coma_amd -Wl,-rpath,/opt/rocm/lib -o run_text
 *     run_text model.sdm ids.bin embeddings_out.bin */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "coma_hip.h"
#include "sd_hip.h"

#define CHECK(x)                                                                      \
  do {                                                                                \
    if ((x) != 0) { fprintf(stderr, "%s failed: %s\n", #x, coma_last_error()); return 1; } \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: run_text model.sdm ids.bin embeddings_out.bin\n"); return 2; }
  void* m = NULL;
  hipStream_t s;
  if (hipStreamCreate(&s) != hipSuccess) return 1;
  CHECK(sd_model_load(argv[1], &m));
  size_t n_ids = 0, n_out = 0;
  void* p = NULL;
  CHECK(sd_model_binding(m, "ids", &p, &n_ids));
  CHECK(sd_model_binding(m, "text_out", &p, &n_out));
  FILE* f = fopen(argv[2], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  int32_t* ids_h = (int32_t*)malloc(n_ids);
  if (fread(ids_h, 1, n_ids, f) != n_ids) { fprintf(stderr, "%s: expected %zu bytes\n", argv[2], n_ids); return 2; }
  fclose(f);
  void *ids = NULL, *out = NULL;
  if (hipMalloc(&ids, n_ids) != hipSuccess || hipMalloc(&out, n_out) != hipSuccess) return 1;
  if (hipMemcpy(ids, ids_h, n_ids, hipMemcpyHostToDevice) != hipSuccess) return 1;
  for (int rep = 0; rep < 2; ++rep) CHECK(sd_text_encode(m, (const int32_t*)ids, out, s));   /* second call = graph replay */
  if (hipStreamSynchronize(s) != hipSuccess) return 1;
  void* out_h = malloc(n_out);
  if (hipMemcpy(out_h, out, n_out, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out_h, 1, n_out, f) != n_out) return 1;
  fclose(f);
  printf("text: %d launches, %zu id bytes, %zu output bytes\n", sd_model_num_launches(m, "text"), n_ids, n_out);
  free(ids_h);
  free(out_h);
  (void)hipFree(ids);
  (void)hipFree(out);
  CHECK(sd_model_destroy(m));
  return 0;
}
