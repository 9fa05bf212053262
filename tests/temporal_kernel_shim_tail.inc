
// every pixel in turn; mode 1: temporalIntegrate< true >, 0: < false >
extern "C" void run_motion(int w,int h,const int* face,const float4* position,const float4* normal,const uint4* facesV,const float4* V,const float4* Hv,float4* motion,float4* reference){
  for(int y=0;y<h;y++) for(int x=0;x<w;x++){ blockIdx.x=x; blockIdx.y=y; threadIdx.x=threadIdx.y=0; ptd::temporalMotion(w,h,face,position,normal,facesV,V,Hv,motion,reference); } }
extern "C" void run_integrate(int mode,const ptd::TemporalArgs* A,float4* working,const float4* position,const float4* normal,const float4* albedo,
  const float4* pI,const float4* pP,const float4* pN,const float4* pA,const unsigned* pL,unsigned* L,float4* info,const float4* motion,const float4* reference){
  for(int y=0;y<A->height;y++) for(int x=0;x<A->width;x++){ blockIdx.x=x; blockIdx.y=y; threadIdx.x=threadIdx.y=0;
    if(mode) ptd::temporalIntegrate<true>(*A,working,position,normal,albedo,pI,pP,pN,pA,pL,L,info,motion,reference);
    else ptd::temporalIntegrate<false>(*A,working,position,normal,albedo,pI,pP,pN,pA,pL,L,info,motion,reference); } }
