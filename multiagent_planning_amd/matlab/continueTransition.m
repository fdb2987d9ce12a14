function [pk,vk,ak,K_T_used,scene_status] = continueTransition(po,pf,prm,K_T_max,error_tol,col0,start)
% Start in motion (no reference counterpart): dmpc_mex('transition', ..) whose column 0 is a carried or given state and plan instead of initDMPC.
% po: 3 x N (or 1 x 3 x N); pf: 3 x N_cmd (N_cmd < N: the vehicles behind the commanded ones are static obstacles).  prm: a dmpc_params_struct.
% Without `start` the flight continues where the last transition of this context ended (the state and every agent's plan are carried on the
% device; the commanded columns of po are ignored); col0 (default 0) is added to that flight's last column.
% start: a struct with the fields vo, ao (3 x N_cmd, [] = zeros), plan_p (3 x K x N_cmd, [] = the braking plan) and plan_v, plan_a (both or []),
% e.g. what [x_p,x_v,x_a,plan_p,plan_v,plan_a,col] = dmpc_mex('flight_end', prm, N_cmd) returned: the flight starts from (po, vo, ao) and column 0
% is the caller's column col0 (scripted windows and the disturbance count from it).
% pk, vk, ak (3 x K_T_max x N_cmd), K_T_used, scene_status: as 'transition'; the columns are this flight's own, column 0 the start.
po = reshape(po,3,[]); pf = reshape(pf,3,[]);
if nargin < 6 || isempty(col0), col0 = 0; end
if nargin < 7
    [pk,vk,ak,K_T_used,scene_status] = dmpc_mex('transition_from', prm, po, pf, K_T_max, error_tol, [], [], [], [], [], col0, 1);
else
    [pk,vk,ak,K_T_used,scene_status] = dmpc_mex('transition_from', prm, po, pf, K_T_max, error_tol, start.vo, start.ao, start.plan_p, start.plan_v, start.plan_a, col0);
end
end
